// pbd_internal.h -- shared declarations of the HIP implementation behind include/pbd.h.
// gfx950 (MI355X) only.  Not part of the public interface.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pbd.h"
#include "pbd_layout.h"

namespace pbd {

// One pyramid level as the kernels see it.  Offsets are per frame; a frame's slice of a buffer
// starts at frame * (per-frame total).
struct LevelDesc {
    int img_rows, img_cols;   // level image (pixels)
    int blk_rows, blk_cols;   // HOG blocks = round(dim / sbin)             (src/HOGFeatures.cpp:174), sbin the LEVEL's (below)
    int rows, cols;           // feature / response map = blocks - 2         (:175), plus the pad on every side
    int padx, pady;           // cells of padding left and right / above and below the map (pbd_set_padding); 0 on an empty level
    int src_level;            // pyrDown source level (level - interval), -1 for resized levels; an index into the table the pyramid
                              // kernels are given, which starts at the plan's first reference level (fine levels own no image)
    int tab_x, tab_y;         // offsets into the resize tables (levels < interval)
    int sbin;                 // the level's bin size: the model's, or half of it on a level of the fine octave (pbd_set_fine_octave)
    long long img_off;        // pixel offset of the level image (multiply by channels for bytes); a fine level shares its base level's
    long long blk_off;        // block offset
    long long cell_off;       // cell offset
    long long quad_off;       // offset in units of 4 consecutive cells of a level (combine step)
};

// resize tables (cv::resize INTER_LINEAR 8U fixed point)
struct ResizeTabX { int sx; short a0, a1; };
struct ResizeTabY { int y0, y1; short b0, b1; };
// the same mapping with float coefficients (16U / 32F / 64F images); last: sx is the last source column (D = S[sx])
struct ResizeTabXf { int sx, last; float a0, a1; };
struct ResizeTabYf { int y0, y1; float b0, b1; };
// image depths HOGFeatures::pyramid accepts (src/HOGFeatures.cpp:136-146), OpenCV's depth codes
enum { kDepth8U = 0, kDepth16U = 2, kDepth32F = 5, kDepth64F = 6 };
inline size_t depth_size(int depth) { return depth == kDepth8U ? 1 : depth == kDepth16U ? 2 : depth == kDepth32F ? 4 : depth == kDepth64F ? 8 : 0; }

// bilinear cell weights of a pixel coordinate (src/HOGFeatures.cpp:252-259), depends on sbin only
template <typename R> struct HogCoordT { int ip; R v0, v1; };
typedef HogCoordT<float> HogCoord;
typedef HogCoordT<double> HogCoordD;

struct ConvTile { int level; int y0, x0; };
// Tile of the exact 5 x 5 convolution: 64 consecutive positions of the sequence "every strip of four rows of every level of
// every frame of the launch, left to right", as up to kConvMaxSeg runs inside one strip each (pbd_kernels_conv.hip)
constexpr int kConvMaxSeg = 3;
struct ConvSeg { int frame, level, strip, x0; };            // frame: index within the launch
struct ConvSegTile { int nseg; int len[kConvMaxSeg]; ConvSeg seg[kConvMaxSeg]; };
// tile of HOG blocks handled by one workgroup of the fused gradient + histogram kernel: kHogTBX x hog_tile_rows(sbin)
constexpr int kHogTBX = 16;
inline int hog_tile_rows(int sbin) { return sbin <= 4 ? 16 : 8; }
// A run of consecutive levels of one bin size -- what one launch of the histogram kernels covers: levels [lv0, lv1), their blocks
// [blk0, blk1) of the frame and their tiles [tile0, tile1) of the fused kernel's table.  A plan without a fine octave has one.
struct HogGroup { int sbin, lv0, lv1, tile0, tile1; long long blk0, blk1; };

// distance-transform job = (part, mixture) of one tree-depth group.  Its input is ONE plane: the raw
// response of its filter for a leaf part, or the accumulated score (response + children's messages,
// written by the combine step of the deeper group) otherwise.
struct DtJob {
    int plane;                // filter id (from_acc == 0) or global mixture index (from_acc == 1)
    int from_acc;
    int gm;                   // global (part, mixture) index: the job's plane in the persistent pointer buffers IxRaw / IyRaw
    int osx, osy;             // anchor
    double ax, bx, ay, by;    // Quadratic(-w0,-w1), Quadratic(-w2,-w3)  (src/DynamicProgram.cpp:125-127)
};

// mixtures per part the job tables and the register arrays of the combine / root kernels are sized for (the reference has no
// limit, include/Parts.hpp:51-261; Person_26parts has 6, Face_68parts 1)
constexpr int kMaxMix = 16;

// one child part of a combine job
struct ChildDesc {
    int job_begin;            // first DtJob (index within the group) of this child
    int nmix;                 // child mixtures K
    int slot;                 // back-pointer slot of (child, parent mixture 0) = ptr_slot[child]
    int bias_off[kMaxMix];          // biasid[child][mm], mm < K (add the parent mixture)
};

// combine job = one PARENT part: for every parent mixture m
//   acc[m] = response(parent, m); for each child in DESCENDING index order: acc[m] += max_mm(dt[child][mm] + bias)
// (the order of the reference's in-place `parent.score += maxv`, src/DynamicProgram.cpp:95,154-156)
struct CombineJob {
    int child_begin, child_end;   // range in the ChildDesc list, descending child index
    int npar;                     // parent mixtures L
    int acc_plane;                // global mixture index of (parent, mixture 0)
    int filter[kMaxMix];                // response plane of (parent, m)
};

struct RootJob {              // one per component
    int nmix;
    int plane[kMaxMix];             // response plane (filter id) or accumulated-score plane per root mixture
    int from_acc;             // bit mm set: plane[mm] is an accumulated-score plane
    float bias;
};

// Sequential schedule (a filter id used more than once inside a component): the reference keys the accumulated
// scores by FILTER id (src/DynamicProgram.cpp:93,115-119,154-156), so parts sharing a filter see each other's
// contributions in processing order (parts nparts-1 .. 1).  One step = one part per component, and this job is the
// part's contribution to its parent's accumulators, applied in place in parent-mixture order.
struct SeqCombineJob {
    int job_begin;            // first DtJob of the part within the step
    int nmix;                 // the part's mixtures K
    int slot;                 // back-pointer slot of (part, parent mixture 0)
    int bias_off[kMaxMix];          // biasid[part][mm]
    int npar;                 // parent mixtures L
    int target[kMaxMix];            // accumulated-score plane (component * F + filter id of (parent, pm))
    int filter[kMaxMix];            // filter id of (parent, pm): the plane the accumulator starts from
    int init[kMaxMix];              // 1: the accumulator has not been touched yet -> start from the raw response (:155)
};

struct PartWalk {             // argmin tree walk, one per part of a component
    int parent;               // local parent index
    int slot;                 // ptr_slot
    int mix0;                 // global (part, mixture) index of the part's mixture 0
    int ksize[kMaxMix];             // filter size per mixture (xsize == ysize == rows, include/Parts.hpp:185-187)
};

constexpr int kWalkMaxParts = 160;   // parts per component the back-tracking walk holds in LDS (Face_68parts: 68, Person_26parts: 26)
// bytes of one spilled PAIR of envelope-stack entries {T sa, sb, za; unsigned vv;} (natural alignment of T)
constexpr size_t kStkPairF32 = 16, kStkPairF64 = 32;
constexpr int kConvTW = 32, kConvTH = 8, kConvQ = 8;
constexpr int kConvMaxK = 31;        // largest filter side of the generic convolution kernel (the reference has no limit)
// the generic kernel stages its haloed tile in LDS in blocks of channels that fit this budget (launch_conv_stage); one
// channel of the widest filter fits, so its dynamic LDS never exceeds the budget
constexpr size_t kConvLdsBudget = 36 * 1024;
static_assert((size_t)(((kConvTH + kConvMaxK - 1) * (kConvTW + kConvMaxK - 1)) | 1) * sizeof(double) <= kConvLdsBudget,
              "one channel of the widest double tile fits the generic kernel's LDS budget");
#ifndef PBD_CONV3_NW
#define PBD_CONV3_NW 8
#endif
constexpr int kConv3NW = PBD_CONV3_NW;   // waves per workgroup of k_conv3

// ---- launch parameter blocks ---------------------------------------------------------------
// one source frame of a mixed-size call: device pointer, size and row pitch in bytes (a region of a larger image reads it in place)
struct FrameDesc {
    const uint8_t *data;
    int rows, cols;
    long long pitch;
};

struct PyrParams {
    const LevelDesc *lv;
    int nlevels, interval, cn;
    int frame0;                   // first frame of this launch (grid index 0)
    long long pix_per_frame;      // pixels (not bytes) of all level images of one frame
    uint8_t *pyr;                 // [frames][pix_per_frame*cn] elements of the image depth
    const uint8_t *frames;        // [frames][rows*cols*cn] dense
    int rows, cols;
    const ResizeTabX *tabx;
    const ResizeTabY *taby;
    int depth;                    // kDepth8U (fixed-point resampling, the tables above) or 16U / 32F / 64F (tables below)
    const ResizeTabXf *tabxf;
    const ResizeTabYf *tabyf;
    // mixed-size calls (one "virtual frame" whose levels are the frames' pyramids, frame-major; frame0 = 0, one grid row):
    // the levels of one launch as runs of a flat pixel index (run i = level run_lev[i], pixels [run_off[i], run_off[i + 1])),
    // and every frame's source image.  NULL on the equal-size path.
    const int *run_lev;
    const long long *run_off;
    int nruns;
    const FrameDesc *fd;
    const int *lv_frame;          // [nlevels] frame of a virtual level
};

struct HogParams {
    const LevelDesc *lv;
    int nlevels, cn, sbin;
    int frame0;
    long long pix_per_frame, blk_per_frame, cell_per_frame;
    const uint8_t *pyr;
    int depth;                    // image depth of `pyr`
    const void *coord;            // HogCoordT<R>[]
    void *gmag;                   // R [frames][pix_per_frame] gradient magnitude per image pixel
    uint8_t *gori;                // [frames][pix_per_frame] snapped orientation 0..17
    void *hist;                   // R [frames][18][blk_per_frame]
    void *norm;                   // R [frames][blk_per_frame]
    void *feat;                   // R [frames][cell_per_frame*32]
    const ConvTile *htiles;       // block tiles of the fused gradient + histogram kernel ({level, by0, bx0})
    int nhtiles;
    int lv0, lv1;                 // the ranged form of k_hog_hist (one HogGroup of several): its levels and ...
    long long blk0, blk1;         // ... their blocks; sbin and coord are then the group's
};

struct ConvParams {
    const LevelDesc *lv;
    const ConvTile *tiles;        // uniform 32 x 8 tiling (generic and MFMA kernels)
    int ntiles;
    const ConvTile *shaped;       // mixed-shape tiling of the exact 5x5 kernel: 32x8 tiles, then 16x16, then 8x32
    int nshaped[3];
    const ConvSegTile *segtiles;  // the exact / FMA 5x5 kernel's cover of the whole launch (all frames)
    int nsegtiles;
    int F;                        // response planes per cell block (all filters of the bank)
    int nf, Fpad, ksize;          // this launch: filters of one size class, padded to kConvQ, their size
    const int *fmap;              // class-local filter index -> response plane (NULL: identity, the single-class case)
    int groups_per_block;         // filter groups (of kConvQ) handled by one workgroup
    int cblock;                   // generic kernel: channels of the haloed tile staged in LDS at a time (32, or less for large filters)
    // k_conv3: the bank cut into units of 2 / 4 / 6 / 8 filters, weights per unit [32][25][QL]
    const void *wts3;
    const int *unit_f0, *unit_ql; // first filter (class-local index) and filters of a unit
    const int *unit_woff;         // float offset of a unit's weights in wts3
    int nunits, units_per_block;
    int c31_zero;                 // the features come from this library's HOG: channel 31 is 0 in every cell of the image
    const float *c31tab;          // k_conv3: [81 border cases][c31stride] ordered sums of the out-of-image taps' channel-31 weights
    int c31stride;
    int frame0;
    long long cell_per_frame;
    const void *feat;             // R [frames][cell_per_frame*32]
    const void *wts;              // R; 5x5 float kernel: [group][32][tap][8]; generic: [32][k*k][Fpad]
    void *resp;                   // R [frames][cell_per_frame*F], level-major then filter planes (fp16 in PBD_CONV_MFMA_F16 mode)
    int fma;
};

struct DpParams {
    const LevelDesc *lv;
    int nlevels;
    int F, NS, NC, NM;            // filters, pointer slots, components, (part, mixture) pairs
    long long cell_per_frame;
    int frame0;                   // first frame of this chunk (absolute index into resp/msg/ptr buffers)
    const void *resp;             // R, or fp16 when resp_half (PBD_CONV_MFMA_F16: BASELINE configs[4] "fp16 responses")
    int bz_x, bz_y;               // every job of the launch has a linear coefficient of exactly -0.0 (and a != 0) along x / y
    int resp_half;
    void *acc;                    // R [frames][cell_per_frame*NM] accumulated scores of non-leaf parts
    uint8_t *Ik;                  // [frames][cell_per_frame*NS] winning child mixture per (part, parent mixture) slot
    int NJ;                       // planes per cell block of IxRaw / IyRaw (= (part, mixture) pairs of the model)
    int ptr8;
    // group scratch, indexed by chunk-local frame
    int JG;                       // jobs in this group
    void *tmp, *dt;               // R [chunk][cell_per_frame*JG]
    long long quad_per_frame;
    int max_mix;                  // largest number of mixtures of any part of the model (<= kMaxMix)
    int lane_shift;               // distance-transform passes: 64 >> lane_shift rows (columns) per wave (set per launch)
    // the transform's own pointers, row-major, KEPT for the whole batch ([frames][cell_per_frame*NJ], plane = DtJob::gm; uint8
    // when ptr8, else int16): IxRaw from the rows pass (stored TRANSPOSED, [x][y], as that pass writes it), IyRaw[y][x] from the columns pass.  The reference's Ix / Iy of a
    // (part, parent mixture) slot are Ix = IxRaw[k][y][x], Iy = IyRaw[k][y][Ix] with k = Ik (include/DistanceTransform.hpp:233-244,
    // src/DynamicProgram.cpp:146-152); only the candidates' walks and pbd_dp_min's read-back ever need them, so they are
    // composed there instead of for every cell
    void *IxRaw, *IyRaw;
    void *stk;                    // [chunk][JG][stk_per_jf] records of two entries, wave-private, lane-interleaved
    long long stk_per_jf;         // records per (job, frame)
    const long long *stk_row_off; // per rows-pass wave (64 flat rows): first entry
    const long long *stk_col_off; // per columns-pass wave
    const DtJob *jobs;
    const ChildDesc *childs;
    const CombineJob *cjobs;
    const SeqCombineJob *sjobs;   // sequential schedule only
    const float *biasw;
    const int *row2level; const int *rowoff;   // flat row -> level, level -> first flat row
    const int *col2level; const int *coloff;
    int nrows_flat, ncols_flat;
    int longest;                  // longest row / column of the plan (LDS of the cooperative passes)
    void *rootv; int *rooti;      // R / int [frames][cell_per_frame*NC]
    const RootJob *rjobs;
};

struct ArgminParams {
    const LevelDesc *lv;
    int nlevels, NS, NC, nframes;
    long long cell_per_frame;
    const void *rootv; const int *rooti;   // rootv: R
    const void *IxRaw, *IyRaw; const uint8_t *Ik;     // see DpParams
    int NJ;
    int ptr8;
    int walk_mode;                // PBD_WALK_* of the handle at enqueue (walk_child)
    float thresh;
    const float *scales;          // [nlevels]
    const PartWalk *walk;         // all components concatenated
    const int *walk_off;          // [NC+1]
    int max_parts, stride, capacity;
    // the candidate list as it leaves the device ("payload"): word 0 = number of roots FOUND (may exceed `capacity`), then
    // min(found, capacity) records of `stride` words in (frame, level, component, y, x) order
    int32_t *payload;
    int *blk; int nblk;           // hits per block of the find kernels, then their exclusive prefix sums
    long long ntotal;             // nframes * cell_per_frame * NC root cells
    int frame_offset;             // added to the `frame` field of every record (frames sharded over GPUs: global frame id)
    // mixed-size calls: virtual level -> (frame of the call, level of that frame's pyramid); NULL: the record's own frame / level
    const int *lv_frame, *lv_local;
    const uint8_t *root_max;      // pbd_set_root_nms: a byte per root cell, laid out as rootv; a hit also needs it non-zero (NULL: off)
    const uint8_t *root_ok;       // pbd_set_depth_prune: likewise, the cells whose box size agrees with the depth image (NULL: off)
    const uint8_t *root_top;      // pbd_set_top_k: likewise, the K best cells of each frame among those the two above leave (NULL: off)
};

// per-frame sort + non-maxima suppression of an argmin payload (pbd_set_nms; pbd_kernels_post.hip)
struct PostParams {
    const int32_t *in;            // payload: word 0 = candidates found, then the records grouped by frame (`frame` frame-local)
    int in_cap;                   // records the input holds; found > in_cap -> output word 0 = -1
    int stride, max_parts, nframes;
    int rows, cols, wpr;          // frame size; canvas words per row = ceil(cols / 32)
    float overlap;
    // workspace, in_cap entries each (fkept: nframes)
    float *key; int *frame; int4 *box; int *perm; int *slot; int *fkept;
    uint32_t *canvas;             // nframes bit canvases of rows * wpr words when they do not fit in LDS
    int32_t *out; int out_cap;    // output payload: word 0 = kept count, then min(kept, out_cap) records
    int frame_offset;             // added to the `frame` field of every emitted record
    // mixed-size calls: per frame {rows, cols} and the word offset of its canvas in `canvas` (NULL: the scalars above, canvas
    // f at f * rows * wpr); `flist` = the frames of one k_post_nms launch (NULL: blockIdx.x), those of one canvas kind
    const int2 *fdim;
    const long long *fcanvas;
    const int *flist;
    // pbd_suppress*: a record's frame is its `frame` field - in_offset; `bad` (NULL: not checked) is set on the device when word 0
    // is negative or a frame index is out of range or not grouped ascending -- then, as on an overflow, word 0 = -1
    int in_offset;
    int *bad;
};

// 3-D box of each record from a depth image (pbd_boxes3d; pbd_kernels_depth.hip)
constexpr int kB3Taps = 35;                   // getGaussianKernel(35, 4) filtered with [-1 0 1]^T (include/Candidate.hpp:190-193)
constexpr int kB3MaxBoxes = kWalkMaxParts + 1;   // the parts, then boundingBoxNorm()
constexpr int kB3MaxGrid = 2048;              // workgroups of one launch (one record each, grid-stride over the rest)
// one depth frame: device pointer, size and row pitch in bytes (a region of a larger image reads it in place), and the size of
// the colour frame its records were detected in
struct Box3dFrame {
    const uint8_t *data;
    int rows, cols;
    long long pitch;
    int im_rows, im_cols;
};
struct Boxes3dParams {
    const int32_t *in;            // payload: word 0 = records (negative: none), then the records
    int in_cap;                   // records the payload holds: min(max(word 0, 0), in_cap) are read
    int stride, max_parts;
    const Box3dFrame *frames;     // [nframes]; a record's frame is its `frame` field - frame_offset
    int nframes, frame_offset;
    int depth;                    // kDepth8U / 16U / 32F / 64F, one per call
    double *out;                  // [record][6]: x, y, z, height, width, depth (Rect3d member order, include/Rect3.hpp:53-64)
    float dog[kB3Taps];           // the derivative-of-Gaussian taps, computed on the host (boxes3d_taps)
};

// camera boxes and part centres of each record (pbd_boxes3d_camera; pbd_kernels_cloud.hip)
enum { kPartsLiteral = 0, kPartsXY = 1 };     // PBD_PARTS_LITERAL / PBD_PARTS_XY
struct Pinhole { double fx, fy, cx, cy, tx, ty; };   // pbd_pinhole
struct CameraParams {
    const int32_t *in;            // the payload of k_boxes3d
    int in_cap, stride, max_parts;
    const Box3dFrame *frames;     // the depth frames (32F) and colour sizes
    const Pinhole *cams;          // [nframes]
    int nframes, frame_offset, mode;
    const double *cube;           // [record][6]: what k_boxes3d wrote
    double *box;                  // [record][6]: the camera box, Rect3d member order
    float *centres;               // [record][max_parts][3]
    int32_t *ncentres, *dense;    // [record]
};

// object clusters of camera boxes in point clouds (pbd_cluster_objects; pbd_kernels_cloud.hip)
constexpr int kClChunk = 1024;                // points of one crop block (4 rounds of 256)
constexpr int kClMaxGrid = 4096;              // workgroups of a grid-stride launch
struct CloudFrame {                           // pbd_cloud, the point pointer and strides as read on the device
    const uint8_t *data;
    int rows, cols;
    long long point_stride, row_stride;
};
struct ClusterParams {
    const int32_t *in;            // payload: word 0 = boxes (negative: none); box i's frame = in[1 + i * rec_stride] - frame_offset
    int in_cap, rec_stride, frame_offset;
    const CloudFrame *clouds;
    int nclouds, nchunks;         // chunks of kClChunk points per box (the largest cloud's)
    const double *boxes;          // [box][6] camera boxes, Rect3d member order
    int crop_cap, index_cap;
    // workspace (pbd_capi_post.hip sizes it from crop_cap / boxes / nchunks: cluster_pieces)
    long long *chunk_off;         // [in_cap * nchunks + 1]: cropped points per chunk, then their exclusive scan
    long long *part;              // scan partials
    int32_t *crop_idx, *crop_box; // [crop_cap]: the point index and the box of every cropped point
    float4 *crop_xyz;             // [crop_cap]
    int32_t *bucket, *parent, *csize;   // [crop_cap]: hash bucket, union-find parent, component size (roots)
    int32_t *sorted;              // [crop_cap]: cropped points in bucket order
    int32_t *bstart, *bcur;       // [tcap + 1]: bucket starts, scatter cursors
    int tcap;                     // buckets allocated (power of two >= 2 crop_cap)
    unsigned long long *best;     // [in_cap]: (size << 32) | ~root of the kept cluster
    long long *obase;             // [in_cap]: first output index of every box
    long long *ntab;              // [4]: cropped total, bucket count, (boxes of the payload) * nchunks, -
    // outputs
    float *centres;               // [box][3]
    int32_t *counts, *indices;
    long long *status;            // [2]: cropped points, output indices (-1: the crop overflowed)
};

// organized multi-plane segmentation of organized clouds (pbd_remove_planes; pbd_kernels_planes.hip)
constexpr int kPlRefLds = 4096;               // rows whose refinement exchange lives in LDS (larger clouds: p.xch)
struct PlaneCloud {                           // pbd_cloud as read on the device, and where it sits in the call's concatenation
    const uint8_t *data;
    int rows, cols;
    long long point_stride, row_stride;
    long long base;               // first point (sum of the earlier clouds' points)
    long long rbase;              // first row (sum of the earlier clouds' rows): the cloud's slice of xch
};
struct PlaneParams {
    const PlaneCloud *clouds;     // [nclouds + 1]: the last entry's base is the call's point total
    int nclouds;
    long long npts;               // points of all clouds
    int half;                     // window half size s = smoothing size / 2
    float depth_change, dist_thr, cos_thr;
    double max_curv;
    int min_inliers, plane_cap, cand_cap;
    // workspace (pbd_capi_post.hip sizes it: plane_pieces)
    float4 *xyz;                  // [npts] the points
    float4 *rsx, *rsy;            // [npts] row sums of the x / y gradients (w of rsx: 1 when the row window holds a depth edge)
    float4 *nrm;                  // [npts] normal and d = n . P
    int32_t *parent, *csize;      // [npts] union-find parent (final: the root), component size (roots)
    int32_t *flag;                // [npts + 1] flags, then their exclusive scan
    int32_t *lab;                 // [npts] working labels: plane index, -2 a finite point of no plane, -1 not finite
    long long *part;              // scan partials
    int32_t *cand_root, *cand_plane, *plane_cnt;   // [cand_cap]
    float4 *cand_coef, *plane_coef;                // [cand_cap]
    int32_t *cbase, *np;          // [nclouds + 1] first candidate of every cloud, [nclouds] planes of every cloud
    int2 *xch;                    // [2 * rows of all clouds] the refinement wavefront's exchange of clouds taller than kPlRefLds
    // outputs
    float *points;                // [npts][3] cloud i at base_i: kept points, then NaN points
    int32_t *kept, *nkept, *labels, *inliers, *nplanes;
    float *planes;                // [nclouds][plane_cap][4]
    long long *status;            // [2]: kept points of all clouds, most planes of one cloud
};

// depth consistency of each record's parts (pbd_depth_consistency*; pbd_kernels_consistency.hip)
constexpr int kDcWaveKeys = 1024;     // samples of a median one wave holds in registers
constexpr int kDcBlockKeys = 4096;    // samples of a median one 256-thread workgroup holds in registers; larger boxes stream
constexpr int kDcMaxGrid = 4096;
struct DcParams {
    const int32_t *in;            // payload: word 0 = records (negative or > in_cap: output word 0 = -1), then the records
    int in_cap;
    int stride, max_parts;
    const Box3dFrame *frames;     // [nframes] depth images (im_rows / im_cols unused); a record's frame is `frame` - frame_offset
    int nframes, frame_offset;
    int depth;                    // kDepth8U / 16U / 32F / 64F, one per call
    int NC;
    const int *part_offset;       // [NC + 1]
    const int *parent;            // [totparts] component-local parent (root -1)
    const double *norm;           // [totparts] norm of the part's mixture-0 anchor (root 0)
    float zfactor;
    // workspace: a median per (record, part) (NaN: empty box), one work list of task_cap entries in three class segments
    // (qn[0..2] their lengths, qn[3..5] the placing cursors), a kept flag per record, a kept count per 256 records
    double *med;
    int *queue, *qn;
    long long task_cap;
    int *flag, *blk;
    int32_t *out; int out_cap;    // output payload: word 0 = kept count, then min(kept, out_cap) records
};
enum { kDcStepClassify = 0, kDcStepSelect, kDcStepCompact, kDcSteps };

// grid maxima of a set of planes (pbd_grid_nms*, pbd_set_root_nms; pbd_kernels_gridnms.hip)
struct GnPlane {
    long long off;                // first element of the plane in src / mask / dst (of a frame)
    long long blk0;               // blocks of the planes before it (an empty plane shares its successor's)
    int rows, cols;
    int nbx, pad;                 // blocks per row of blocks: ceil(cols / (sz + 1))
};
struct GridNmsParams {
    const GnPlane *planes;        // [nplanes] the planes of one frame
    int nplanes, nframes;         // every frame has the same planes, frame_stride elements apart
    long long frame_stride, blocks_per_frame;
    const void *src;              // R
    const uint8_t *mask;          // NULL: every element that is not NaN is eligible
    int use_thresh;               // the detect path: eligible = src > (R)thresh; with a mask, those of them whose byte is non-zero
    float thresh;
    int sz;
    uint8_t *dst;                 // 0 / 255, every byte of every plane written
};
// plane `off`, rows x cols, cut into blocks of sz + 1: its table entry; *blocks = the blocks so far, advanced by the plane's
inline GnPlane grid_nms_plane(long long off, int rows, int cols, int sz, long long *blocks)
{
    const long long bs = (long long)sz + 1, nbx = (cols + bs - 1) / bs, nby = (rows + bs - 1) / bs;
    const GnPlane g{off, *blocks, rows, cols, (int)nbx, 0};
    *blocks += nbx * nby;
    return g;
}
// scale-depth plausibility of a root box (pbd_set_depth_prune, pbd_depth_prune*; pbd_kernels_depthprune.hip)
struct DepthPruneRule { double fx, width, tol; };   // pbd_depth_prune_cfg, widened
struct DepthPruneRoots {          // the plane form, next to the call's ArgminParams
    const Box3dFrame *frames;     // [frames of the call] depth images; a mixed-size call's virtual level gives the frame
    int depth;                    // kDepth8U / 16U / 32F / 64F
    DepthPruneRule rule;
    uint8_t *ok;                  // 1 / 0 per root cell, laid out as rootv; every byte written
};

// scale NMS of the root cells (pbd_set_scale_nms; pbd_kernels_scalenms.hip), next to the call's ArgminParams
struct ScaleNmsRoots {
    int dl;                       // neighbouring levels on either side, 0..255
    const uint8_t *root_ok;       // pbd_set_depth_prune's byte per root cell (NULL: off)
    const uint8_t *root_max;      // pbd_set_root_nms's byte per root cell (NULL: off)
    uint8_t *dst;                 // 255 (eligible and kept) / 0 per root cell, laid out as rootv; every byte written
};

// the K best elements of every segment of a packed array (pbd_top_k_cells*, pbd_set_top_k; pbd_kernels_topk.hip)
constexpr int kTkTile = 1024;     // elements per tile; every segment is cut into tiles of its own
struct TopKTab {                  // [nseg + 1]: a segment's first element and first tile; entry nseg holds the totals
    long long off, tile0;
};
struct TopKSeg {                  // a segment's selection so far: the key digits fixed, the elements still to take among the
    unsigned long long prefix;    // keys that share them.  After the last pass: the pivot key and the pivot-valued elements kept
    int need, done, pad;          // done: settled in pass 0 (K = 0 or K >= eligible)
};
struct TopKParams {
    const TopKTab *tab;           // NULL: nseg segments of ulen elements and utiles tiles each (the detect path's equal frames)
    int nseg, k;
    long long ulen, utiles, ntiles;
    const void *src;              // R
    const uint8_t *mask;          // NULL: every element that is not NaN is eligible
    const uint8_t *mask2;         // the detect path: a second byte plane (root NMS after depth pruning)
    int use_thresh;               // the detect path: eligible = src > (R)thresh, and the mask bytes where given
    float thresh;
    uint8_t *dst;                 // 0 / 255, every byte written
    int *hist;                    // [nseg * 256] zero on entry and on exit
    TopKSeg *state;               // [nseg]
    int *tcnt;                    // [ntiles + 1]
    long long *part;              // [top_k_scan_parts(ntiles)]
};
inline long long top_k_tiles(long long len) { return (len + kTkTile - 1) / kTkTile; }

constexpr int kGnWaveSz = 7;      // sz below it: one lane per block; from it on: one wave per block (profiles/grid_nms/README.md)

// ---- kernel launches and their timing -------------------------------------------------------
// Every kernel of the library is launched through PBD_LAUNCH.  While a profiling scope is open on the calling thread
// (pbd_profile_enable; bench.py's roofline figures) the launch carries a start / stop event pair of its own
// (hipExtLaunchKernelGGL): the timestamps are those of the kernel's dispatch packet, so nothing is inserted into the stream
// between kernels.  (Bracketing a kernel with hipEventRecord puts a marker packet on either side of it: 10.5 us per
// kernel boundary in the rocprofv3 trace of round 3, 0.45 ms of every 64-frame step -- profiles/r03_hd/README.md.)
struct ProfHook {
    void *ctx;
    void (*take)(void *ctx, hipEvent_t *start, hipEvent_t *stop);
};
extern thread_local ProfHook *g_prof_hook;

template <typename F, typename... Args>
inline void launch_k(F kernel, const dim3 &grid, const dim3 &block, unsigned lds, hipStream_t s, Args... args)
{
    hipEvent_t a = nullptr, b = nullptr;
    if (g_prof_hook) g_prof_hook->take(g_prof_hook->ctx, &a, &b);
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, a, b, 0, args...);
}
#define PBD_LAUNCH(kernel, grid, block, lds, stream, ...) ::pbd::launch_k(kernel, grid, block, lds, stream, __VA_ARGS__)

// ---- launchers (pbd_kernels_*.hip) ---------------------------------------------------------
void launch_resize(const PyrParams &p, int nframes, long long npix_resized, hipStream_t s);
void launch_pyrdown_range(const PyrParams &p, int nframes, int first_level, int last_level, long long base,
                          long long npix, hipStream_t s);
// mixed-size calls: the levels listed in p.run_lev / p.run_off (all resized levels of every frame, or one octave of every
// frame), p.run_off[p.nruns] pixels, in one launch
void launch_resize_runs(const PyrParams &p, hipStream_t s);
void launch_pyrdown_runs(const PyrParams &p, hipStream_t s);
// `f64` selects the reference's T=double instantiation (every real-typed buffer then holds doubles)
// pass 1 of the two-pass form over the level images `p.lv` (reference levels only: every image once); then, per HogGroup, the
// histograms: the fused kernel (`fused`, only where hog_fused() holds), else pass 2 (`ranged`: the group is not the whole plan)
bool hog_fused(const HogParams &p, bool f64);
void launch_hog_grad(const HogParams &p, int nframes, bool f64, hipStream_t s);
void launch_hog_hist(const HogParams &p, int nframes, bool f64, bool fused, bool ranged, hipStream_t s);
void launch_hog_feat(const HogParams &p, int nframes, bool f64, bool padded, hipStream_t s);
void launch_conv(const ConvParams &p, int nframes, bool f64, hipStream_t s);
int conv_occupancy(int nw);
int conv_mfma_occupancy(bool f16);
// matrix-core path (pbd_kernels_conv_mfma.hip); wrec: [pass][tap][160 filters][144 B] bf16 hi/lo records
// PBD_CONV_MFMA_F16: 80 B fp16 records, one MFMA per product tile
void launch_conv_mfma(const ConvParams &p, const void *wrec, bool f16, int nframes, hipStream_t s);
constexpr int kMfmaFilterBlock = kWrecFilterBlock, kMfmaRecBytes = 144, kMfmaRecBytesF16 = 80;
// PBD_CONV_MFMA_F64 (pbd_kernels_conv_mfma_f64.hip).  A size class of nf filters is ceil(nf / 16) M-tiles, split into passes
// (grid y) by the pass rule of pbd_layout.h (mfma_passes, mfma_pass_begin).
// wfrag: the class's A-fragments in the order of f64_frag_source (pbd_layout.h); the channel block of a filter size is
// conv_mfma_f64_qn(): 4 * qn channels per block
constexpr size_t kF64LdsTarget = 80 * 1024;   // haloed tile per workgroup: two workgroups per CU (160 KB of LDS)
int conv_mfma_f64_qn(int ksize);
size_t conv_mfma_f64_lds(int ksize, int qn);
void launch_conv_mfma_f64(const ConvParams &p, const double *wfrag, int nframes, hipStream_t s);
// PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY (pbd_kernels_conv_mfma_any.hip): the float matrix-core path for any filter side, one
// launch per size class.  wfrag: the class's A-fragments in the order of any_frag_source (pbd_layout.h).  The haloed 32 x 8
// tile is staged in blocks of conv_mfma_any_cb() channels: the largest of 32 / 16 / 8 whose tile fits kAnyLdsTarget (two
// workgroups per CU); 8 channels of the widest filter take 113 KB (bf16) and leave one.
constexpr size_t kAnyLdsTarget = 80 * 1024;
inline size_t conv_mfma_any_lds(int ksize, int cb, bool f16)
{
    return (size_t)(kConvTW + ksize - 1) * (kConvTH + ksize - 1) * (cb * (f16 ? 2 : 4) + 16);
}
inline int conv_mfma_any_cb(int ksize, bool f16)
{
    int cb = 32;
    while (cb > 8 && conv_mfma_any_lds(ksize, cb, f16) > kAnyLdsTarget) cb /= 2;
    return cb;
}
static_assert((size_t)(kConvTW + kConvMaxK - 1) * (kConvTH + kConvMaxK - 1) * (8 * 4 + 16) <= 160 * 1024,
              "8 channels of the widest filter's tile fit the CU's LDS");
int conv_mfma_any_occupancy(int ksize, bool f16);
void launch_conv_mfma_any(const ConvParams &p, const void *wfrag, bool f16, int nframes, hipStream_t s);
// The dynamic-LDS limit of every variant of k_conv_mfma_any / k_conv_mfma_f64, raised on the CURRENT device; their one caller
// is conv_prepare_device (pbd_capi.hip)
hipError_t conv_mfma_any_set_lds_limits();
hipError_t conv_mfma_f64_set_lds_limits();
// the convolution modes by what they imply (every site that used to compare with the enum values asks these)
inline bool conv_is_f16(int mode) { return mode == PBD_CONV_MFMA_F16 || mode == PBD_CONV_MFMA_F16_ANY; }        // fp16 operands and resident responses
inline bool conv_is_matrix_f32(int mode) { return mode == PBD_CONV_MFMA || mode == PBD_CONV_MFMA_ANY || conv_is_f16(mode); }   // float handle, matrix cores
inline bool conv_is_any(int mode) { return mode == PBD_CONV_MFMA_ANY || mode == PBD_CONV_MFMA_F16_ANY; }         // every filter size
// the distance-transform passes' launch choices a handle may force (pbd_debug_set_option); the defaults decide per launch
struct DtOptions {
    int lane_shift = -1;          // 0..6: 64 >> lane_shift rows (columns) per wave; -1: by the launch's size
    bool coop = true;             // false: never the wavefront-cooperative kernel k_dt_coop
    int coop_g = 0;               // 4 or 8: rows per wave of k_dt_coop; 0: by the launch's size
};
void launch_dt_rows(const DpParams &p, const DtOptions &o, int nframes, bool f64, hipStream_t s);
void launch_dt_cols(const DpParams &p, const DtOptions &o, int nframes, bool f64, hipStream_t s);
void launch_dp_combine(const DpParams &p, int ncjobs, int nframes, bool f64, hipStream_t s);
void launch_dp_combine_seq(const DpParams &p, int nsjobs, int nframes, bool f64, hipStream_t s);
void launch_dp_root(const DpParams &p, int nframes, bool f64, hipStream_t s);
void launch_argmin_find(const ArgminParams &p, bool f64, hipStream_t s);
int argmin_find_span();       // root cells per block of the find kernels (sizes ArgminParams::blk)
void launch_argmin_walk(const ArgminParams &p, bool f64, hipStream_t s);
bool post_canvas_in_lds(int rows, int cols);
size_t post_canvas_words(int rows, int cols);
void launch_postprocess(const PostParams &p, hipStream_t s);
// mixed-size calls: frames lds_frames[0..nlds) with their canvases in LDS (the largest lds_words words), glb_frames[0..nglb)
// with theirs in p.canvas
void launch_postprocess_mixed(const PostParams &p, const int *lds_frames, int nlds, size_t lds_words, const int *glb_frames,
                              int nglb, hipStream_t s);
// `grid` workgroups (capped at kB3MaxGrid), each computing one record at a time
void launch_boxes3d(const Boxes3dParams &p, int grid, hipStream_t s);
// one step of the depth-consistency filter (kDcStep*, in this order); dc_record_blocks: workgroups of the compaction (p.blk entries)
void launch_depth_consistency(const DcParams &p, bool f64, int step, hipStream_t s);
int dc_record_blocks(int in_cap);
// the compaction alone: the records whose p.flag is set (p.blk: their count per dc_record_blocks block) into p.out, in order
void launch_dc_emit(const DcParams &p, hipStream_t s);
// p.root_ok's bytes for every root cell of the call (a.ok): above the threshold and plausible under a.rule
void launch_depth_prune_roots(const ArgminParams &p, const DepthPruneRoots &a, bool f64, hipStream_t s);
// the record form: p.flag / p.blk from each record's root rectangle (p.in, p.frames, p.depth), then launch_dc_emit
void launch_depth_prune_records(const DcParams &p, const DepthPruneRule &rule, hipStream_t s);
// the grid maxima of p's planes; lanes per block: grid_nms_lanes(sz, forced) = 1 or 64 (forced: 0 = by sz)
int grid_nms_lanes(int sz, int forced);
void launch_grid_nms(const GridNmsParams &p, bool f64, int lanes, hipStream_t s);
// the scale-space maxima of the call's root cells into a.dst
void launch_scale_nms_roots(const ArgminParams &p, const ScaleNmsRoots &a, bool f64, hipStream_t s);
// the record form: p.flag / p.blk from the rule over each record's frame, then launch_dc_emit
void launch_scale_nms_records(const DcParams &p, int dl, hipStream_t s);
// the K best eligible elements of every segment of p (4 passes for float, 8 for double, then the ordered mark); the long longs of
// p.part
long long top_k_scan_parts(long long ntiles);
void launch_top_k(const TopKParams &p, bool f64, hipStream_t s);
// the record form: p.flag / p.blk from each record's rank among its frame's records by score, then launch_dc_emit
void launch_top_k_records(const DcParams &p, int k, hipStream_t s);
// camera boxes and part centres of p.in's records (after launch_boxes3d wrote p.cube)
void launch_camera_boxes(const CameraParams &p, hipStream_t s);
// one step of the clustering (kClStep*, launched in this order); nothing is read back
enum { kClStepCropCount = 0, kClStepCropScan, kClStepCropScatter, kClStepClear, kClStepGridCount, kClStepGridScan, kClStepGridScatter,
       kClStepHook, kClStepLabel, kClStepBest, kClStepSelect, kClStepOut, kClSteps };
void launch_cluster_step(const ClusterParams &p, int step, hipStream_t s);
// organized multi-plane segmentation (kPlStep*, launched in this order; refine = 0 skips kPlStepRefine); nothing is read back
enum { kPlStepLoad = 0, kPlStepRowSums, kPlStepNormals, kPlStepHook, kPlStepSize, kPlStepCand, kPlStepCandScan, kPlStepCandList,
       kPlStepMoments, kPlStepPlanes, kPlStepLabel, kPlStepRefine, kPlStepFinal, kPlStepKeptScan, kPlStepKept, kPlStepOut, kPlSteps };
void launch_planes_step(const PlaneParams &p, int step, hipStream_t s);

// candidate mask and masked frame (pbd_candidate_mask*; pbd_kernels_publish.hip)
struct MaskFrame {
    uint8_t *labels;              // rows x cols labels, label_pitch bytes apart (NULL: not written)
    const uint8_t *colour;        // rows x cols pixels of `channels` bytes, colour_pitch apart (read only when masked is set)
    uint8_t *masked;              // the masked frame (may be colour itself, same pitch); NULL: not written
    long long label_pitch, colour_pitch, masked_pitch;
    int rows, cols;
    int tile0;                    // the frame's first tile in the call's numbering
};
struct MaskParams {
    const int32_t *in;            // payload: word 0 = records (negative or > in_cap: a bad list), then the records
    int in_cap, stride, max_parts;
    const MaskFrame *frames;      // [nframes]; a record's frame is its `frame` field - frame_offset
    int nframes, frame_offset, ntiles, channels;
    int4 *hull;                   // [in_cap] workspace: each record's clipped hull x0, y0, x1, y1 (all 0: empty)
    int32_t *range;               // [2 * nframes] workspace: each frame's first and end record
    int32_t *bad;                 // [1] workspace: the list is bad
    int32_t *status;              // the device form's status word (-1 or the record count); NULL: none
};
enum { kMkStepHull = 0, kMkStepTile };
void launch_mask(const MaskParams &p, int step, hipStream_t s);
long long mask_tiles(int rows, int cols);   // k_mk_tile's tiles of one frame

// the part-centre pose of each record (pbd_part_poses*; pbd_kernels_publish.hip)
struct PoseParams {
    const int32_t *count_word;    // min(max(word 0, 0), cap) records
    int cap, max_parts;
    const float *centres;         // [record][max_parts][3]
    const int32_t *ncentres, *dense;
    int32_t *count;               // [record]
    float *position, *orientation, *eigenvalues;   // [record][3], [record][4] (x, y, z, w), [record][3]
};
void launch_part_poses(const PoseParams &p, hipStream_t s);

// testing a model (pbd_part_nms*, pbd_best_overlap*, pbd_eval_pck*, pbd_eval_apk*; pbd_kernels_eval.hip)
constexpr int kEvMaxBoxes = 1000;   // nms.m's cut, the largest max_boxes
struct EvalNmsParams {
    const int32_t *in;            // payload: word 0 = records (negative or > in_cap: a bad list), then the records
    int in_cap, stride, nparts, nframes, frame_offset, max_boxes;
    int row_words;                // ceil(max_boxes / 64): 64-bit words of a row of the suppression matrix
    float overlap;
    int32_t *frame;               // [in_cap] workspace: each record's frame index
    uint32_t *key;                // [in_cap] ordered score keys
    int32_t *bad;                 // [1] the list is bad (zeroed by the caller)
    int32_t *order;               // [nframes][max_boxes] record index by pick rank
    double *hull;                 // [nframes][max_boxes][4] x1, y1, x2, y2 of the rank's hull
    unsigned long long *bits;     // [nframes][max_boxes][row_words]: bit j of row i = pick rank i removes rank j (j > i)
    int32_t *slot;                // [nframes][max_boxes] position among the frame's kept records, or -1
    int32_t *fm, *fkept;          // [nframes] records after the cut, records kept
    int32_t *out; int out_cap;    // output payload: word 0 = kept count (-1: bad list), then min(kept, out_cap) records
};
enum { kEvNmsSelect = 0, kEvNmsPairs, kEvNmsGreedy, kEvNmsEmit, kEvNmsSteps };
void launch_eval_nms(const EvalNmsParams &p, int step, hipStream_t s);
struct EvalBestParams {
    const int32_t *in;
    int in_cap, stride, nparts, nframes, frame_offset;
    float overlap;
    const double *gtbox;          // [nframes][4] x1, y1, x2, y2 (a NaN: no ground truth)
    unsigned long long *best;     // [nframes] workspace, zeroed by the caller
    int32_t *out, *found;         // [nframes][stride], [nframes]
};
void launch_eval_best(const EvalBestParams &p, hipStream_t s);
struct EvalPckParams {
    const int32_t *rec, *found;   // [nframes][stride], [nframes]
    int stride, nparts, nframes;
    const double *gt, *scale;     // [nframes][nparts][2], [nframes]
    double thresh;
    double *pck, *dist;           // [nparts], [nparts][nframes] or NULL
};
void launch_eval_pck(const EvalPckParams &p, hipStream_t s);
struct EvalApkParams {
    const int32_t *in;
    int in_cap, stride, nparts, nframes, frame_offset, G, list_cap;
    const int32_t *gt_offset;     // [nframes + 1]
    const double *gt, *gscale;    // [G][nparts][2], [G]
    double thresh;
    uint32_t *key;                // [in_cap] workspace
    int32_t *order;               // [in_cap] record index by rank
    int32_t *close;               // [in_cap][nparts] the instance within thresh of (rank, part), or -1
    int32_t *first;               // [G][nparts] earliest rank that is close to the instance (set to a large value by the caller)
    int32_t *tplist;              // [nparts][list_cap] ranks of the true positives
    double *mp;                   // [nparts][list_cap] their running maximum of the precision from the end
    double *apk, *prec, *rec;     // [nparts], [nparts][in_cap] or NULL
    int32_t *status;              // record count, or -1 for a bad count
};
enum { kEvApkRank = 0, kEvApkClose, kEvApkAp, kEvApkSteps };
void launch_eval_apk(const EvalApkParams &p, int step, hipStream_t s);

// training examples of records (pbd_examples*; pbd_kernels_examples.hip)
struct ExPart {                   // one (example, part), written by the walk, read by the gather
    long long cell;               // first cell of the part's level in `feat` (frame * cell_per_frame + cell_off)
    long long dst;                // element offset of the filter block in `values`
    int x, y, m, k;               // position, mixture and filter size (k = 0: no block)
    int W, H, pad0, pad1;         // the level's feature map
};
struct ExGm { int filterid, biasid, defid, pad; };   // per (part, mixture) of the model
struct ExampleParams {
    const int32_t *in;            // payload: word 0 = records (negative: none), then the records
    int in_cap, stride, frame_offset;
    const LevelDesc *lv;
    int nlevels, nframes;         // equal-size plans: frames of the batch
    const int *frame_lv0;         // mixed plans: [nframes + 1] first virtual level of each frame (NULL: equal-size plan)
    long long cell_per_frame;
    int NC, NS, NJ, ptr8, flen, max_parts;
    int walk_mode;                // PBD_WALK_* of the handle at the call (walk_child)
    const int *rooti;
    const void *IxRaw, *IyRaw; const uint8_t *Ik;   // see DpParams
    const PartWalk *walk; const int *walk_off;
    const ExGm *gm;
    const int *anchors;           // [ndefs][2]
    const long long *foff;        // [nfilters] offset of each filter in the model vector
    int nbias, ndefs;
    const void *feat;             // R [frames][cell_per_frame * flen]
    ExPart *parts;                // [in_cap * max_parts] workspace
    int32_t *hdr; int hdr_words;
    void *values; int vstride;
};
void launch_examples(const ExampleParams &p, bool f64, int step, hipStream_t s);   // step 0: walk, 1: gather

// part scores of records (pbd_part_scores*, pbd_score_placements*; pbd_kernels_partscores.hip)
struct PartScoreParams {
    const int32_t *in;            // payload: word 0 = records (negative: none), then the records
    int in_cap, stride, frame_offset;
    const LevelDesc *lv;
    int nlevels, nframes;         // equal-size plans: frames of the batch
    const int *frame_lv0;         // mixed plans: [nframes + 1] first virtual level of each frame (NULL: equal-size plan)
    long long cell_per_frame;
    int NC, NS, NJ, ptr8, max_parts;
    int walk_mode;                // PBD_WALK_* of the handle at the call (walk_child)
    int F, NM, resp_half;         // planes per cell block of resp (NM: of acc, not read), resp holds fp16
    const void *resp;             // the resident responses (see DpParams)
    void *acc;                    // not read (LevelPlanes::score names it)
    const int *rooti;
    const void *IxRaw, *IyRaw; const uint8_t *Ik;   // see DpParams
    const PartWalk *walk; const int *walk_off;
    const int *part_nmix;         // [parts of the model] mixtures of a part, indexed as `walk`
    const ExGm *gm;               // per (part, mixture): filter id in `resp`, bias id, deformation id
    const int *anchors;           // [ndefs][2]
    const float *defw;            // [ndefs][4]
    const float *biasw;
    const int32_t *place_in;      // pbd_score_placements*: [in_cap][max_parts][3] x, y, m given by the caller (NULL: the walk's)
    int32_t *status;              // [in_cap] parts of the record, or -1
    int32_t *place;               // [in_cap][max_parts][3]
    void *scores;                 // R [in_cap][max_parts][4] appearance, message, bias, total
};
void launch_part_scores(const PartScoreParams &p, bool f64, int step, hipStream_t s);   // step 0: placements, 1: scores

// max-marginals of every part (pbd_max_marginals, pbd_marginal_poses*; pbd_kernels_marginals.hip).  The
// planes of ONE frame: mm / down T, Jx / Jy int16, Jk int8, each [cell_per_frame * NJ] with a level's block [gm][y][x] from its
// cell offset on; msg T [cell_per_frame * NS], one plane per pointer slot (part, parent type).
struct MmSlot {                   // k_mm_messages: one part p of an upward depth group, its message to every parent type
    int job_begin, nmix;          // p's first transform of the group (the group's dt scratch), its types
    int slot, npar;               // the message planes written: slot + mq, mq < npar (the parent's types)
    int bias_off[kMaxMix];        // biasid of (p, m)
};
struct MmCtx {                    // k_mm_context: one context plane (part p, parent type mq) of a slice
    int filter;                   // the response plane of (q, mq)
    int sib_begin, sib_end;       // range in the sibling list: message planes slot(c) + mq, c descending, c != p
    int down;                     // the down plane of (q, mq): global (part, type) index
    int out;                      // the context plane written (index within the slice)
};
struct MmRun {                    // k_mm_down: parent types [mq0, mq1) of part p, whose transforms are one slice's jobs from job0 on,
    int job0, nmix;               // ordered (mq, m); p's types
    int mq0, mq1, npar;           // npar: the parent's types; mq0 > 0 resumes from the planes an earlier slice left
    int gm0;                      // global index of (p, 0): the planes written
    int s_from_acc;               // S_p[m] is the accumulated plane gm0 + m, else the response plane s_filter[m]
    int s_filter[kMaxMix];
    int bias_off[kMaxMix];
};
// (a root is a run with npar == 0: down_0[m] = (T)biasw[bias_off[0]] for every m, -1 in its pointer planes)
struct MmParams {
    const LevelDesc *lv;
    int nlevels;
    int F, NS, NC, NM, NJ;        // as DpParams (NJ: the (part, type) pairs = planes of the outputs)
    long long cell_per_frame, quad_per_frame;
    int frame;                    // the frame of the resident result
    int ptr8;                     // the resident pointer planes hold uint8
    const void *resp; const void *acc;               // the resident result (R)
    const uint8_t *Ik; const void *IxRaw, *IyRaw;    // the resident upward pointers (k_mm_decode)
    const float *biasw;
    // the call's scratch, frame 0: dt = the transforms' values [cells * JG], sIx / sIy their pointer planes [cells * SJ] (plane =
    // job index), ctx = the context planes [cells * JG]
    const void *dt; const void *sIx, *sIy; void *ctx;
    int JG, SJ, NCTX;             // planes per cell block of dt, of sIx / sIy, of ctx in this launch
    int max_mix;
    // the frame's planes
    void *msg, *mm, *down; int16_t *Jx, *Jy; int8_t *Jk;
    const MmSlot *slots; const MmCtx *ctxs; const int *sibs; const MmRun *runs;
    // k_mm_decode
    const PartWalk *walk; const int *walk_off; const int *part_nmix;
    const float *scales;
    const int32_t *seeds; int nseeds, stride, max_parts, frame_offset;
    int32_t *cand, *place, *status;
};
void launch_mm_messages(const MmParams &p, int nslots, bool f64, hipStream_t s);
void launch_mm_context(const MmParams &p, int nctx, bool f64, hipStream_t s);
void launch_mm_down(const MmParams &p, int nruns, bool f64, hipStream_t s);
void launch_mm_decode(const MmParams &p, bool f64, hipStream_t s);

// latent positives (pbd_detect_latent; pbd_kernels_examples.hip).  The responses are those of the latent bank: one plane per
// (component, part, mixture) = global mixture index gm, so a mask belongs to its (component, part, mixture).
struct LatentParams {
    void *resp;                   // R [cell_per_frame * F] of the call's virtual frame (mixed plan)
    const LevelDesc *lv;
    int nlevels, F;               // F = planes per cell block = (part, mixture) pairs of the model
    long long cell_per_frame;
    const int *lv_frame;          // virtual level -> frame of the call
    const float *scales;          // [nlevels]
    int resp_half;                // resp holds fp16 (conv_is_f16): the mask value is kLatentMaskHalf
    const int4 *gmtab;            // [F] {part index in its component, mixture, filter size, -}
    const int4 *boxes;            // [nframes][nparts] ground truth {x1, y1, x2, y2}, inclusive
    const int *mix;               // [nframes][nparts] fixed mixture or -1 (NULL: all free)
    int nparts;
    double overlap;
    // the per-frame arg-max
    const void *rootv; const int *rooti;
    const int *frame_lv0;         // [nframes + 1]
    int nframes, NC, stride;
    int32_t *payload;             // word 0 = nframes, then one record per frame (as k_argmin_emit writes them, for the walk)
};
// A masked response is -1e10 in T (Matlab's -INF, finite).  fp16 resident responses hold the most negative finite half instead;
// a root score that uses a masked term is then below kLatentFoundHalf as long as its other terms sum to less than 32752.
constexpr float kLatentMaskHalf = -65504.0f, kLatentFoundHalf = -32752.0f;
void launch_latent_mask(const LatentParams &p, bool f64, hipStream_t s);
void launch_latent_best(const LatentParams &p, bool f64, hipStream_t s);

// warped positives (pbd_warp_positives*; pbd_kernels_warp.hip).  Kept box j is level j of a plan of `nkept` P x P level images
// (image j at pixel j * P * P of the pyramid buffer, its k x k cells at cell j * k * k of the feature buffer): k_warp writes the
// images, the HOG launches of the detect path turn them into features, k_warp_emit writes every box's example.
struct WarpTap { int i0, i1; };   // the two source columns of a destination column: window taps, clamped into the frame
struct WarpParams {
    const FrameDesc *fd;          // the call's frames
    const int *box_frame;         // [nkept] frame of kept box j
    const WarpTap *tapx;          // [nkept][P]
    const void *cx, *cy;          // [nkept][P] coefficients: ResizeTabX / ResizeTabY (8U) or ResizeTabXf / ResizeTabYf; the y0, y1
                                  // of cy are the two source rows, clamped into the frame; sx of cx is not used
    int nkept, P, cn, depth;
    uint8_t *pyr;                 // [nkept][P][P][cn] elements of the image depth
    // k_warp_emit
    int nboxes;
    const int *slot;              // [nboxes] the kept index j of box i, -1: skipped
    int bias;                     // the bias block's offset in w, -1: none
    int filter_off, filter_len;   // the filter block in w: nbias + 4 ndefs + filter_offset[filter], k * k * flen
    const void *feat;             // R [nkept][filter_len]
    int32_t *hdr; int hdr_words;
    void *values; int vstride;
    int32_t *payload;             // word 0 = nboxes, then record i (NULL: the host form, no payload)
    int rec_stride, id_offset;
};
void launch_warp(const WarpParams &p, hipStream_t s);
void launch_warp_emit(const WarpParams &p, bool f64, hipStream_t s);

// augmented positives (pbd_augment_frames*; pbd_kernels_augment.hip).  A job is one destination image:
// rotate(mirror(source)), nearest neighbour.  A tile is kAugTileCols consecutive pixels of kAugTileRows consecutive destination
// rows of one job; the tile table runs over every job of the call.
constexpr int kAugTileCols = 256, kAugTileRows = 8;
struct AugJob {
    const uint8_t *src; uint8_t *dst;
    long long spitch, dpitch;     // bytes between rows
    int srows, scols, drows, dcols;
    int mirror, rotate;           // rotate 0: degrees == 0, the destination has the source's size and no coordinate is computed
    double c, s, hAr, hAc, hBr, hBc;
};
struct AugTile { int job, y0, x0; };
struct AugParams {
    const AugJob *jobs;
    const AugTile *tiles;
    int ntiles, cn, depth;
};
void launch_augment(const AugParams &p, hipStream_t s);

// the training QP (pbd_qp_*; pbd_kernels_qp.hip).  One cache entry i: x[i * V ..] float values in stored block order, bm[i * V ..]
// the block of every value, hd[i * HW ..] = {nblocks, nvalues, (offset in w, length, first value) x nblocks}, ids[i * 5 ..],
// b, d, a (double) and sv (uint8).  Every kernel runs PBD_QP_LANES threads per workgroup (the lanes of the header's reduction).
struct QpCache {
    float *x; uint8_t *bm; int32_t *hd; int32_t *ids;
    double *b, *d, *a; uint8_t *sv;
    int cap, V, HW, MB;           // capacity, values per entry, header words, most blocks of an entry (<= 256)
    double *w; const double *wreg, *w0;
    const int *noneg; int nnoneg, L;
    const int *slot_of;           // [L] the layout block starting at a coordinate, -1 elsewhere
    const int *slot_len;          // [layout blocks] its length
};
struct QpWriteParams {
    QpCache c;
    const int32_t *in_hdr; const void *in_values; int in_hw, in_vs;   // pbd_examples' format and strides
    const int32_t *in_ids;        // [m][5] (pbd_qp_add), or NULL: ids from the payload's records
    const int32_t *payload; int rec_stride, label, id_base;          // pbd_qp_add_device
    int m, n0;                    // examples of the call (payload: its capacity), entries before the call
    double Cpos, Cneg;
    int *slot;                    // [m] entry of each example, -1: skipped
    int *taken; int32_t *taken_user;
};
void launch_qp_write(const QpWriteParams &p, bool f64, hipStream_t s);
struct QpPassParams {
    QpCache c;
    const int *order, *gidx;      // [nsteps] entry and group of every step
    int nsteps, ngroups;
    double *idC; int *idI; double *err;   // [ngroups]
    double *loss;                 // out: the sum of err in group order
};
void launch_qp_pass(const QpPassParams &p, hipStream_t s);
struct QpScoreParams {
    QpCache c;
    const double *w;              // the weights scored
    const int *list; int first, count;   // entries list[k] (NULL: first + k)
    int sub_b; double scale;      // out[k] = sub_b ? R(w . x) - b : R(w . x) / scale
    double *out;
};
void launch_qp_score(const QpScoreParams &p, hipStream_t s);
struct QpTask { int off, c0, n, begin, end, pad; };   // lincomb: coordinates off + c0 .. + n of one layout block
struct QpLincombParams {
    QpCache c;
    const QpTask *tasks; int ntasks;
    const int2 *ent;              // {entry, first value of the block in the entry}, ascending a within a task's range
    double *ww;                   // out (k_qp_norm): R(w . w) after the non-negativity clamps
};
void launch_qp_lincomb(const QpLincombParams &p, hipStream_t s);   // w = 0, the sums, the clamps and R(w . w)
void launch_qp_norm(const QpLincombParams &p, hipStream_t s);      // the clamps and R(w . w) only
void launch_qp_wraw(const QpCache &c, double *out, hipStream_t s);   // out = w + w0 .* wreg
struct QpGatherParams {
    QpCache c;
    const int *src; int count, dst0;    // entry src[k] -> dst0 + k
    float *x; uint8_t *bm; int32_t *hd; int32_t *ids; double *b, *d, *a;   // scratch of `count` entries
};
void launch_qp_gather(const QpGatherParams &p, hipStream_t s);
struct QpHingeParams {            // pbd_qp_add_loss_device
    const int32_t *payload; int capacity, rec_stride;
    double y, Cl;                 // +1 / Cpos or -1 / Cneg
    double *out;                  // [1] Cl * R(max(0, 1 - y * score)) over the records present
};
void launch_qp_hinge(const QpHingeParams &p, hipStream_t s);

// part types by k-means (pbd_cluster_parts*; pbd_kernels_kmeans.hip).  A pair = (part, trial), pair = part * trials + trial.
constexpr int kKmMaxGrid = 2048;     // workgroups of k_km_trials (one pair each, grid-stride over the rest)
struct KmPart { int a, b, K, root; };   // X[n] = def[a][n] - def[b][n]; the part's types; 1 for the root (anchors 0)
struct KmParams {
    const double *def;            // [nparts][npos][2]
    const KmPart *parts;          // [nparts]
    const int32_t *start;         // [pairs][kMaxMix] the point each centroid starts at (the first K of a pair are read)
    int nparts, npos, trials, max_iter;
    // workspace, per pair
    uint8_t *lab;                 // [pairs][npos] labels
    double *sumdist; int32_t *iters;   // [pairs]
    double *cen; int32_t *cnt;    // [pairs][kMaxMix][2], [pairs][kMaxMix]
    // outputs (k_km_pick)
    int32_t *idx;                 // [nparts][npos]
    double *centres;              // [nparts][kMaxMix][2]
    int32_t *counts, *anchors;    // [nparts][kMaxMix], [nparts][kMaxMix][2]
    pbd_cluster_info *info;       // [nparts]
};
void launch_km_trials(const KmParams &p, int maxK, hipStream_t s);   // maxK: the largest K of the call
void launch_km_pick(const KmParams &p, hipStream_t s);

// in-place model update (pbd_set_model_vector*, pbd_qp_apply; pbd_kernels_model.hip).  Every kernel returns at once when
// *refused is set (k_mu_check found a deformation whose quadratic term rounds to zero), so a refused call writes nothing.
enum { kMuSrcF32 = 0, kMuSrcF64 = 1, kMuSrcQp = 2 };
struct MuSource {                 // the new vector: L values of float / double, or the QP's w_k / wreg_k + w0_k in double
    const void *w;
    const double *wreg, *w0;
    int code;
};
struct MuJobRef { DtJob *job; int def; int pad; };   // a distance-transform job of any group and its deformation
struct MuParams {
    int *refused;                 // word 0 of the status block
    float *st_bias, *st_def;      // the status block's copy of the float32 bias and deformation values
    int L, nbias, ndefs, totmix, NC, njobs;
    const int *gm_def;            // [totmix] the deformation of a non-root (part, mixture), -1 for a root's
    const int *root_bias;         // [NC]
    void *mvec;                   // R [L] the handle's model vector on the device
    float *biasw; RootJob *rjobs; const MuJobRef *jobs;
    const long long *foff;        // [nfilters] offset of filter f in the model vector
};
struct MuClassParams {            // one size class of the bank
    const int *refused;
    const void *mvec; const long long *foff;
    const int *fmap;              // class-local index -> filter id (NULL: identity)
    int K, nf, Fpad, group_layout;
    void *wts;
    float *wts3; const int *unit_f0, *unit_ql, *unit_woff; int nunits;
    float *c31tab; int c31stride;
    double *wfrag64; int qn;
    uint16_t *wrec; int wrec_f16, nfilters;   // the matrix-core records (one class, filter ids in order)
    uint16_t *wfrag16; int any_cb;            // PBD_CONV_MFMA_*_ANY: the class's A-fragments, their channel block (wrec_f16: fp16)
};
void launch_mu_check(const MuParams &p, const MuSource &src, hipStream_t s);
void launch_mu_vector(const MuParams &p, const MuSource &src, bool f64, hipStream_t s);   // mvec, the status block's values
void launch_mu_tables(const MuParams &p, bool f64, hipStream_t s);                        // d_biasw, root biases, DtJobs
void launch_mu_class(const MuClassParams &p, bool f64, hipStream_t s);                    // every table of the class that is set

}  // namespace pbd
