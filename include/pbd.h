/*
 * pbd.h -- C ABI of the MI355X-native PartsBasedDetector detection hot path.
 *
 * Drop-in boundary: each entry point states the reference interface it replaces (paths relative to
 * the reference repository).  Plain C, no OpenCV/STL/torch types; every pointer is a host pointer
 * unless the name says `_device`.  Functions return PBD_OK (0) or a negative pbd_status; the text of
 * the last failure on a handle is available from pbd_last_error().  No exception crosses this ABI.
 *
 * Layouts at the seam are the reference's:
 *   image    rows x cols x channels, uint8, interleaved BGR (channels 3) or grey (channels 1)
 * T below is the handle's real type: float for PBD_REAL_F32 (src/demo.cpp:85), double for PBD_REAL_F64
 * (cells/detect.cpp:93, ros/Node.hpp:121); real-typed buffers cross the ABI as void pointers to T.
 *   feature  Mat(H, W*flen) single-channel T, channel fastest        (src/HOGFeatures.cpp:180,288)
 *   filter   Mat(k, k*flen) T, same interleave                       (src/MatlabIOModel.cpp:115-123)
 *   response Mat(H, W) T, one per (level, filter): responses[level][filter]
 *
 * One handle = one host thread = one GPU (as the reference's detector is not re-entrant:
 * src/HOGFeatures.cpp:99-107).  The library fails if the HIP runtime or device is unavailable; there
 * is no CPU fallback.
 */
#ifndef PBD_H_
#define PBD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBD_MAX_LEVELS 128

typedef enum pbd_status {
    PBD_OK = 0,
    PBD_ERR_INVALID = -1,     /* bad argument / model fails validation (reference: assert / CV_Error) */
    PBD_ERR_UNSUPPORTED = -2, /* e.g. image depth other than 8-bit (src/HOGFeatures.cpp:136-146 default branch) */
    PBD_ERR_HIP = -3,         /* HIP runtime error */
    PBD_ERR_CAPACITY = -4,    /* candidate capacity exceeded; output truncated */
    PBD_ERR_STATE = -5,       /* call order violated (e.g. pdf before setFilters) */
    PBD_ERR_NOMEM = -6
} pbd_status;

/* Flattened Model + Parts tables (include/Model.hpp:49-122, include/Parts.hpp:51-261).
 * gp = part_offset[c] + p is a global part index; gm = mix_offset[gp] + m a global (part, mixture)
 * index.  Copied at pbd_create (the reference's Parts copies the pools: include/Parts.hpp:232-235). */
typedef struct pbd_model {
    int ncomponents;
    int nfilters;
    int flen;                      /* channels per HOG cell (32) */
    const int *filter_ksize;       /* [nfilters]; filter f is k x k x flen */
    const int64_t *filter_offset;  /* [nfilters] element offset of filter f in filters_f32/_f64 */
    const float *filters_f32;      /* used when real_type == PBD_REAL_F32 */
    const double *filters_f64;     /* used when real_type == PBD_REAL_F64 (may be NULL otherwise) */
    int nbias;
    const float *biasw;            /* [nbias] */
    int ndefs;
    const float *defw;             /* [ndefs*4] */
    const int *anchors;            /* [ndefs*2] (x, y), 0-based */
    const int *part_offset;        /* [ncomponents+1] */
    const int *parentid;           /* [totparts], root -1; parent index < child index */
    const int *mix_offset;         /* [totparts+1] */
    const int *filterid;           /* [totmix] */
    const int *biasid;             /* [totmix]: biasid_[c][p][mm]; bias(mm)[m] = biasw[biasid + m] (Parts.hpp:172-175) */
    const int *defid;              /* [totmix]: defid_[c][p][mm] (root: ignored) */
    float thresh;
    int sbin;
    int interval;                  /* Model::nscales_ (src/FileStorageModel.cpp:105) */
    int norient;                   /* 18 */
} pbd_model;

enum { PBD_REAL_F32 = 0, PBD_REAL_F64 = 1 };
enum { PBD_CONV_EXACT = 0,   /* multiply and add rounded separately in the reference's order: bit-identical responses */
       PBD_CONV_FMA = 1,     /* fused multiply-add: responses within 1e-4 on unit-scale inputs, not bit-identical.
                                Relative to M = sum |w| |f| over the response's window (border cells included) and
                                K = k*k*32 products, every response is within 8 sqrt(K) u M of the exact sum, u = 2^-24
                                (float) or 2^-53 (double; against the reference's own double sum: twice that) -- under
                                0.02 of that bound observed (tests/conv_reference.py, tests/test_gpu_conv_modes.py) */
       PBD_CONV_MFMA = 2,    /* matrix cores, bf16 hi/lo operand split (3 MFMAs per product tile), fp32 accumulation:
                                responses within 1e-4 on unit-scale inputs, not bit-identical; every response within
                                8 sqrt(3K) 2^-24 M of the exact sum of hi*hi + hi*lo + lo*hi (lo*lo, ~2^-16 of a product,
                                is not computed) -- under 0.04 of that bound observed, RMS relative error ~2^-26;
                                5x5 filters, PBD_REAL_F32 only */
       PBD_CONV_MFMA_F16 = 3 }; /* matrix cores, operands rounded once to fp16 (1 MFMA per product tile), fp32 accumulation:
                                the 1e-4 bar does not hold (~1e-3 observed on unit-scale scores); same restrictions.
                                Every response is within 8 sqrt(K) 2^-24 M of the exact sum of the fp16 operands'
                                products, plus half an fp16 ulp of the result (the response's own rounding).
                                In this mode the RESPONSES live on the device as fp16 (BASELINE configs[4] "fp16 responses"):
                                pbd_conv_pdf returns them widened to float, |v| >= 65520 saturates to +-inf (accepted by the
                                dynamic program: see "Non-finite scores" at pbd_dp_min), and pbd_dp_min
                                ROUNDS THE CALLER'S float scores to fp16 before the dynamic program (exact for scores that
                                came from pbd_conv_pdf; arbitrary scores lose precision: tests/test_gpu_parity.py::
                                test_mfma_f16_dp_min_rounds_its_input pins this) */
enum { PBD_CONV_MFMA_F64 = 4 };  /* fp64 matrix cores (v_mfma_f64_16x16x4_f64), fp64 operands and fp64 accumulation:
                                responses within fp64 rounding of the reference's summation order (~1e-13 relative;
                                within 2 * 8 sqrt(K) 2^-53 M of the reference's double responses, as PBD_CONV_FMA),
                                not bit-identical; every filter size the exact path takes; PBD_REAL_F64 only (pbd_create
                                refuses it for PBD_REAL_F32 with PBD_ERR_UNSUPPORTED) */

enum { PBD_CONV_MFMA_ANY = 5,       /* the arithmetic of PBD_CONV_MFMA for every filter size 1..31 and mixed banks */
       PBD_CONV_MFMA_F16_ANY = 6 }; /* the arithmetic and the fp16 resident responses of PBD_CONV_MFMA_F16, likewise.
                                Operands are emulated exactly as in modes 2 / 3.  bf16 mode: every fp32 operand is split
                                x = hi + lo with round-to-nearest-even and hi*hi + hi*lo + lo*hi is accumulated in fp32 by
                                v_mfma_f32_32x32x16_bf16.  fp16 mode: every operand is rounded once to fp16, one
                                v_mfma_f32_32x32x16_f16 per product tile, fp32 accumulation; the response is stored as fp16
                                and |v| >= 65520 becomes +-inf.  Bound: each response lies within 8 sqrt(n) 2^-24 M of the
                                float64 sum of the emulated products, n = 3 k k 32 (bf16) or k k 32 (fp16, plus half an fp16
                                ulp of the result), M = sum |w| |f| over the window, border cells included.  The constant
                                border is 0, and 1 on channel 31; where M == 0 the response is exactly 0.  One launch per
                                size class, the filter side a runtime value; an all-5x5 bank runs the kernel and weight
                                records of modes 2 / 3, so mode 5 equals mode 2 and mode 6 equals mode 3 bit for bit there.
                                PBD_REAL_F32 only: pbd_create refuses both for PBD_REAL_F64 with PBD_ERR_UNSUPPORTED
                                (that real type has PBD_CONV_MFMA_F64).  pbd_detect_latent in mode 6 masks with the most negative
                                finite fp16 value (see there); mode 3 keeps refusing it. */

typedef struct pbd_config {
    int device;            /* HIP device ordinal */
    int real_type;         /* PBD_REAL_F32 (src/demo.cpp:85) or PBD_REAL_F64 (cells/detect.cpp:93) */
    int conv_mode;         /* PBD_CONV_EXACT / _FMA / _MFMA / _MFMA_F16 / _MFMA_F64 / _MFMA_ANY / _MFMA_F16_ANY */
    int max_batch;         /* frames per pbd_detect_batch* call (>= 1) */
    int max_candidates;    /* candidate capacity per batch */
    void *stream;          /* hipStream_t to run on (NULL: the library creates its own) */
} pbd_config;

/* One detection = one reference Candidate (include/Candidate.hpp:56-80): parts_ as x,y,w,h,
 * confidence_[0] = score, component_.  The reference's walk leaves the other parts' confidences 0
 * (src/DynamicProgram.cpp:241-244) and a record carries none; pbd_part_scores* compute them from the resident result.
 * A record is pbd_candidate_stride() int32 words: this header followed by max_parts x {x,y,w,h}. */
typedef struct pbd_candidate_hdr {
    int32_t frame;      /* index within the batch */
    int32_t component;
    int32_t level;
    int32_t root_x;
    int32_t root_y;
    float score;
    int32_t nparts;
    int32_t reserved;
} pbd_candidate_hdr;

typedef struct pbd_handle pbd_handle;

/* ---- lifetime.  Replaces PartsBasedDetector<T>::distributeModel (src/PartsBasedDetector.cpp:102-127). */
int pbd_create(const pbd_model *model, const pbd_config *config, pbd_handle **out);
void pbd_destroy(pbd_handle *h);
const char *pbd_last_error(const pbd_handle *h); /* h may be NULL: last error of a failed pbd_create */
const char *pbd_version(void);
int pbd_candidate_stride(const pbd_handle *h);  /* int32 words per candidate record */

/* ---- IFeatures (include/IFeatures.hpp:49-73), implemented by HOGFeatures<T> (src/HOGFeatures.cpp). */
int pbd_binsize(const pbd_handle *h);                      /* IFeatures::binsize */
/* Plans the pyramid for a rows x cols frame: level image sizes, feature map sizes and scales
 * (src/HOGFeatures.cpp:95-127,174-175).  Replaces the size/scale logic of HOGFeatures::pyramid and
 * IFeatures::nscales()/scales().  Arrays hold PBD_MAX_LEVELS entries. */
int pbd_pyramid_plan(pbd_handle *h, int rows, int cols, int *nlevels, int *img_rows, int *img_cols,
                     int *feat_rows, int *feat_cols, float *scales);
/* IFeatures::pyramid(im, pyrafeatures): feat[l] receives feat_rows[l] x (feat_cols[l]*flen) values of T.
 * stride_bytes: byte distance between image rows (cv::Mat::step).  depth_code = cv::Mat::depth() of the image: 0 (CV_8U),
 * 2 (CV_16U), 5 (CV_32F) or 6 (CV_64F) -- the four features<IT> instantiations of src/HOGFeatures.cpp:136-146; any other
 * depth fails with PBD_ERR_UNSUPPORTED as the reference's CV_Error.  A 32F / 64F image holding a NaN or Inf pixel is
 * refused with PBD_ERR_INVALID (here and in pbd_detect_typed): non-finite input is an error, not a silently different result. */
int pbd_features_pyramid(pbd_handle *h, const void *img, int rows, int cols, int channels,
                         size_t stride_bytes, int depth_code, void *const *feat);
/* the resampled level images of the last pbd_features_pyramid / pbd_detect call (for tests), addressed as pbd_get_stage below;
 * PBD_ERR_STATE when the last call that wrote the handle's pyramid was neither: none yet, pbd_conv_pdf and pbd_dp_min (which start
 * from uploaded maps), pbd_detect_latent (whose level images are its twin's) and pbd_warp_positives (whose patches replaced them).
 * pbd_conv_set_filters and a model update leave the level images readable. */
int pbd_get_pyramid_image(pbd_handle *h, int frame, int level, uint8_t *dst);

/* Level sharding (new surface; the reference has no multi-device mode): pyramid levels are independent through HOG,
 * convolution and the dynamic program (src/DynamicProgram.cpp:115-119 reads only scores[n] of the same level), so ONE
 * frame can be split over `world` GPUs -- handle `rank` then computes only its share of the levels (longest-processing-
 * time assignment over the level sizes, the same on every rank) and returns only their candidates; the union over the
 * ranks is the full result.  pbd_pyramid_plan reports 0 x 0 feature maps for the levels of other ranks.  (1, 0..): off.
 * A call that changes neither value leaves the resident result; one that changes the shard drops it (the image plans depend on
 * the shard), and every read-back gives PBD_ERR_STATE until the next detect call. */
int pbd_set_level_shard(pbd_handle *h, int rank, int world);

/* The padded pyramid (new surface; opt-in, off on a new handle).  The Matlab detector pads every feature
 * level by a border of cells holding 0 on channels 0 .. 30 and 1 on channel 31, the boundary occlusion feature
 * (featpyramid.m:36-45), places roots and parts on the larger map and takes the pad off in the box arithmetic
 * (detect.m:266-270); the reference left the call commented out (src/HOGFeatures.cpp:147-148), so that no root or part can lie
 * outside the map.  With padding (padx, pady) every non-empty level of every plan the handle builds AFTERWARDS -- single frame,
 * equal-size batch, pbd_detect_frames*, regions, the _submit / _wait form and pbd_detect_latent* -- is
 * (feat_rows + 2 pady) x (feat_cols + 2 padx) cells: the interior is bit for bit the unpadded plane, a pad cell holds +0 (sign
 * bit clear) on channels 0 .. 30 and 1 on channel 31.  An empty level (too small, or another rank's under level sharding) stays
 * empty.  Convolution in every mode, the distance transforms, the dynamic program, the find, root NMS and top-K run on the padded
 * planes as on any others; everything a plan derives from level sizes (offsets, tile tables, the uint8 / int16 choice of the
 * position planes at a longest side of 256, workspace sizes, the level-shard assignment) derives from the padded sizes.  A
 * part's rectangle of plane cell (x, y) is that of cell (x - padx, y - pady): Point(x - padx - 1, y - pady - 1) * scale, cvRound.
 * root_x / root_y of a record, the cells of pbd_part_scores* / pbd_score_placements*, the windows of pbd_examples* (beyond the
 * padded plane the border rule holds as before) and every plane of pbd_get_stage are in PLANE coordinates; the image cell is
 * root_x - padx.  pbd_pyramid_plan reports the padded feat_rows / feat_cols (image sizes, scales, the level count and the
 * frame-size checks do not change); pbd_features_pyramid writes padded planes.  PBD_CONV_EXACT computes channel 31 like the
 * others on a padded plan (its shortcut needs the channel to be 0 in every cell).  pbd_dp_argmin / pbd_argmin_device_out walk
 * with the pad of the resident plan; after pbd_conv_pdf / pbd_dp_min on the caller's maps that is the handle's setting when
 * they ran: the caller's planes are taken to be padded by it.  Patch plans of pbd_warp_positives* are never padded.
 * pbd_set_nms / pbd_suppress (boxes are cut to the frame as before), pbd_set_walk, pbd_set_root_nms, pbd_set_top_k, level
 * sharding, pbd_detect_latent* (a ground-truth box may lie partly outside the frame) and the post-detection calls that take
 * records and images work on a padded handle.
 * 0 <= padx, pady <= 31 (the largest filter side), else PBD_ERR_INVALID; (0, 0): off.  PBD_ERR_STATE while a batch is in
 * flight.  A call that changes neither value leaves the resident result; one that changes a value drops it and the cached
 * plans, and every read-back gives PBD_ERR_STATE until the next writing call.  A model update keeps the setting.
 * PBD_ERR_UNSUPPORTED (a later change can lift these): a non-zero padding while pbd_set_depth_prune is enabled, and
 * pbd_set_depth_prune(cfg != NULL) while the padding is non-zero; pbd_max_marginals, pbd_get_marginals and pbd_marginal_poses*
 * on a padded resident result. */
int pbd_set_padding(pbd_handle *h, int padx, int pady);

/* The fine octave (new surface; opt-in, off on a new handle; partsbaseddetector_amd/fineoctave.py states
 * the rule in numpy).  The detector's smallest scale is the frame itself at the model's bin size (level 0, plan_pyramid), so an
 * object smaller than the model's template cannot be found.  Felzenszwalb's featpyramid computes the first `interval` levels a
 * second time at bin size sbin / 2 on the SAME resampled images -- an octave of levels at twice the feature resolution; the
 * reference kept only the comment (matlab/detection/featpyramid.m:7).  With the octave on, every image plan the handle builds
 * AFTERWARDS -- single frame, equal-size batch, pbd_detect_frames*, regions, the _submit / _wait form and pbd_detect_latent* --
 * has nfine = min(interval, nlevels) more levels, IN FRONT: level i < nfine is the HOG of reference level i's image at bin size
 * sbin / 2 (blocks = round(dim / (sbin / 2)), feature map = blocks - 2, plus the pad of pbd_set_padding) and its scale is
 * scale[i] / 2 exactly; level nfine + l is the reference's level l, its features, scale and all that is computed from them bit
 * for bit what they were.  No image is resampled anew: pbd_get_pyramid_image(level < nfine) returns the image of level
 * nfine + level, and pbd_pyramid_plan reports nlevels + nfine levels, the fine ones with the image sizes of the levels they
 * share and half their scales.  A record's `level`, the levels of pbd_get_stage, pbd_part_scores* / pbd_score_placements*,
 * pbd_examples*, pbd_features_pyramid and the max-marginal calls index this longer list.  Convolution in every mode, the
 * distance transforms, the dynamic program, the find, root NMS, top-K, depth pruning (its rule reads the level's scale), the
 * walk, suppression, level sharding and padding see only more (and larger) levels; everything a plan derives from level sizes
 * derives from the longer table (the uint8 / int16 choice of the position planes at a longest side of 256 included: a fine
 * level is twice as long as its base level).  Parts at a finer octave than their parent remain out of scope.  Patch plans of
 * pbd_warp_positives* and the explicit-size calls (pbd_conv_pdf, pbd_dp_min) never get the octave.
 * PBD_ERR_STATE while a batch is in flight.  A call that does not change the setting leaves the resident result; one that
 * changes it drops the result and the cached plans, and every read-back gives PBD_ERR_STATE until the next writing call.  A
 * model update keeps the setting; the latent twin follows its handle.
 * PBD_ERR_UNSUPPORTED: enabling it on a model whose sbin is odd or below 4 (the fine bin size must be an integer >= 2, the range
 * the HOG kernels are pinned on); a frame whose plan would exceed PBD_MAX_LEVELS levels (reported by the call that plans it). */
int pbd_set_fine_octave(pbd_handle *h, int enable);

/* Per-frame post-processing (opt-in; off on a new handle): what every caller of the reference runs after detect() --
 * Candidate::sort(candidates) then Candidate::nonMaximaSuppression(im, candidates, overlap) (cells/detect.cpp:237-238,
 * ros/Node.cpp:192-196; include/Candidate.hpp:91-99,277-304) -- on the device, on the handle's stream, after argmin.  Per frame:
 *   sort      by score descending; equal scores keep the device order (a stable sort; -0.0 and +0.0 tie)
 *   suppress  greedily in that order: box = hull of the part rectangles (cv::Rect operator|) & Rect(0, 0, cols, rows);
 *             skip the candidate when (double)painted_pixels_in_box / box.area() > (double)overlap, else paint box and keep it;
 *             an empty box (area 0: NaN ratio) is kept and paints nothing
 * Output: frame by frame (ascending), that frame's kept records in sorted order -- the same records, fewer of them.
 * Applies to pbd_detect, pbd_detect_typed, pbd_detect_batch, pbd_detect_batch_device, pbd_detect_batch_submit / _wait,
 * pbd_detect_batch_device_submit, pbd_detect_batch_device_out and pbd_argmin_device_out; NOT to pbd_dp_argmin (that is
 * DynamicProgram::argmin, which does not suppress).  The stage reads the whole list the handle found (capacity
 * pbd_config.max_candidates), never the caller-truncated one: when more than max_candidates are found the synchronous calls
 * return PBD_ERR_CAPACITY with *ncand = 0 and the device-out payload's word 0 is -1; when only the kept records exceed the
 * caller's capacity the behaviour is that of the unsuppressed list (truncation, PBD_ERR_CAPACITY, word 0 = kept count).
 * enable = 0: off.  A NaN overlap is PBD_ERR_INVALID; PBD_ERR_STATE while a batch is in flight (the setting is latched at
 * submit); PBD_ERR_UNSUPPORTED together with level sharding (world > 1), in either order of the two calls: suppression of one
 * rank's levels is not suppression of the union.  With pbd_set_top_k on, K is taken before the suppression, so fewer than K may
 * survive it; root NMS, scale NMS (pbd_set_scale_nms) and top-K together keep K distinct objects -- root NMS alone works
 * inside one (level, component) plane, so that without scale NMS the K may be one object seen on K neighbouring levels. */
int pbd_set_nms(pbd_handle *h, int enable, float overlap);
/* The walk from a root to its parts (new surface, opt-in).  A child's mixture is m = Ik[slot + pm][py][px] in both modes; with k
 * the plane of that mixture:
 *   PBD_WALK_REFERENCE (the default): x = IxRaw[k][py][px], y = IyRaw[k][py][x] -- the reference's composed pointers
 *     Iy[y][x] = IyRaw[y][Ix[y][x]] (include/DistanceTransform.hpp:233-244).  The placement is usually NOT the one the score was
 *     taken at, so w . x of its example is below the score.
 *   PBD_WALK_ARGMAX: y = IyRaw[k][py][px], x = IxRaw[k][y][px] -- the arg-max of the two passes in the order they ran (the
 *     column pass reads the row pass's output).  w . x of the example equals the score to rounding, the identity detect.m:139-145
 *     asserts and a latent SVM needs of its negative constraints.
 * The mode governs every walk the handle enqueues afterwards: the part boxes of all pbd_detect* records (and so what pbd_set_nms
 * suppresses), pbd_argmin_device_out and pbd_dp_argmin (the resident result is re-walked in the mode current at the call; it is
 * not dropped: the planes are the same), pbd_examples*, and pbd_detect_latent, whose latent twin follows its handle.  Roots,
 * scores, record order and pbd_dp_min's read-back (the reference's composed Ix / Iy) are the same in both modes.
 * Another mode: PBD_ERR_INVALID; while a batch is in flight: PBD_ERR_STATE. */
enum { PBD_WALK_REFERENCE = 0, PBD_WALK_ARGMAX = 1 };
int pbd_set_walk(pbd_handle *h, int mode);

/* Grid maxima of a set of planes (new surface; opt-in): nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129,
 * include/nms.hpp), the block NMS of Neubeck and Van Gool the reference's detect() calls on rootv between min and argmin and leaves
 * commented out (ssp_.nonMaxSuppression(rootv, scales), src/PartsBasedDetector.cpp:86).
 * Planes are packed row-major without padding: plane i (rows[i] x cols[i], M x N below) starts at the sum of rows * cols of the
 * planes before it; `mask` (NULL: none) and `dst` have the same layout; dst receives 0 or 255 in every byte.  rows / cols are
 * host arrays in both forms.  A plane with rows * cols == 0 is legal and produces nothing.  real_code is PBD_REAL_F32 or
 * PBD_REAL_F64, whatever the handle's T: the handle gives the stream, the workspace and the error text only.
 *   eligible      an element that is not NaN and, with a mask, whose mask byte is non-zero
 *   blocks        of (sz + 1) x (sz + 1) elements start at every multiple of sz + 1; the last one in each direction is clipped
 *   candidate     a block's largest eligible element, among equal ones the first in raster order (cv::minMaxLoc)
 *   neighbourhood rows cy - sz .. cy + sz, columns cx - sz .. cx + sz around the candidate (cy, cx), clipped to the plane, MINUS the
 *                 cells of the candidate's own block; only eligible elements count
 *   result        dst = 255 at the candidate iff it is strictly greater than every such neighbour, compared in the plane's own
 *                 type; every other byte is 0.  At most one maximum per block.
 * Decisions where OpenCV's behaviour cannot be pinned from here:
 *   empty block   a block without an eligible element has no maximum (minMaxLoc would report (-1, -1) and the reference would
 *                 write out of bounds)
 *   empty neighbourhood  beats nothing: the candidate is kept (OpenCV returns 0 for an empty mask, which would drop every lone
 *                 maximum with a negative score)
 *   NaN           is never eligible.  +0.0 and -0.0 tie; +Inf against +Inf ties (a tie drops the candidate, and inside a block the
 *                 first of the tied wins)
 *   unmasked      a larger neighbour that is not eligible is ignored, as mask.mul(blockmask) does
 *   These follow the code, not the doc comment of nms.cpp: a constant plane that fits in one block has one maximum, at (0, 0); a
 *   ramp has one, at its far edge; a constant plane spanning several blocks has one, at (0, 0), whose clipped window is its own
 *   block (every other block's candidate ties with a neighbour).  sz = 0 is legal: blocks of 1 x 1, and every
 *   eligible element is kept.  There is no upper bound on sz other than 32767.
 * PBD_ERR_INVALID: sz < 0 or sz > 32767, a negative nplanes / rows / cols, another real_code, or NULL src / dst / rows / cols with
 * nplanes > 0.  PBD_ERR_STATE while a batch is in flight.  The resident detect result is not touched.
 * pbd_grid_nms: host planes, synchronous.  pbd_grid_nms_device: device planes (d_src aligned to its element), asynchronous on
 * pbd_stream(). */
int pbd_grid_nms(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *src, const uint8_t *mask,
                 int sz, uint8_t *dst);
int pbd_grid_nms_device(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *d_src,
                        const uint8_t *d_mask, int sz, uint8_t *d_dst);
/* Root NMS (opt-in; sz = 0, off, on a new handle): with sz in 1..32767 every later detect call first runs the step above over every
 * rootv plane of the call -- one per (frame, level, component) -- with eligibility `rootv > (T)thresh`, the find's own expression
 * (NaN is false), and the find additionally requires the plane's byte.  Result: the same records, fewer of them, in the same
 * (frame, level, component, y, x) order; scores, part boxes and every other word are untouched, and word 0 of a device payload is
 * the kept count.  max_candidates, the caller's capacity, PBD_ERR_CAPACITY and pbd_set_nms see only the kept list.
 * Applies to every entry point pbd_set_nms lists, and to pbd_detect_frames / _device / _device_out.  NOT to pbd_dp_argmin
 * (DynamicProgram::argmin: the reference's call sat in detect, outside it), pbd_examples*' re-walks, or pbd_detect_latent, which
 * has its own best-root search.  Level sharding is allowed: the step is per level, so the union over the ranks is the unsharded
 * result.  Another sz: PBD_ERR_INVALID; while a batch is in flight: PBD_ERR_STATE (the setting is latched at submit). */
int pbd_set_root_nms(pbd_handle *h, int sz);

/* 3-D boxes from a depth image (new surface; opt-in, nothing else calls it): the callers' next step after the suppression above,
 * Candidate::boundingBox3D(im, depth) of every kept candidate (the first step of PointCloudClusterer::computeBoundingBoxes:
 * cells/detect.cpp:224-255, ros/Node.cpp:183-206, include/PointCloudClusterer.hpp:53-77; include/Candidate.hpp:140-216).
 * out[6*i .. 6*i+5] = {x, y, z, height, width, depth} of record i (Rect3d member order, include/Rect3.hpp:53-64).
 * depth[f] is frame f's depth image: one channel, depth_code 0 (8U), 2 (16U), 5 (32F) or 6 (64F), one code per call, any pitch;
 * im_rows[f] x im_cols[f] is the size of the colour frame the records of frame f were detected in (the depth image may have
 * another size).  A record's frame index is its `frame` field minus frame_offset.  Records are this handle's
 * (pbd_candidate_stride), e.g. what any pbd_detect* call returned, with or without pbd_set_nms.  Per record:
 *   boxes    parts[n] & Rect(0, 0, cols, rows) for each part, then boundingBoxNorm() & the same: centroids cvRound((tl + br) * 0.5),
 *            cv::meanStdDev of them in double, Rect(xmean - 1.5 xstd, ymean - 1.5 ystd, 3 xstd, 3 ystd) truncated
 *   scale    x, y, width, height each truncated after the multiplication by dcols / (double)cols or drows / (double)rows
 *   samples  the depth under every box, in box order (overlaps counted twice), as float; valid: != 0 and not NaN (Inf counts).
 *            If the first box of non-zero area has no valid sample: the NaN box {NaN, NaN, NaN, 0, 0, 0}.  If every box has zero
 *            area the reference fails an OpenCV assertion; here that is the NaN box too
 *   result   the sorted samples resized to 400 (cv::resize INTER_LINEAR, float), filtered with the 35-tap derivative of
 *            getGaussianKernel(35, 4); from index 200 walk up and down while |d| <= 0.035: z = p[dmin], depth = p[dmax] - z
 *            (in double); x, y, width, height: boundingBox(), the unclipped hull of the parts
 * pbd_boxes3d: host records and depth images, host output, synchronous.  PBD_ERR_INVALID, naming the index, before anything is
 * enqueued: a depth_code other than the four, a non-positive size, a pitch below the row size, a depth image of more than
 * 2^31 / (max parts + 1) pixels, a record whose frame index is outside 0..nframes-1 or whose nparts is outside 1..max parts.
 * PBD_ERR_STATE while a batch is in flight.
 * pbd_boxes3d_device: d_depth[f].data are device pointers (a frame may be a region of a larger device image, read in place, as
 * the _device frames of pbd_detect_frames_device: pointer and pitch multiples of the element size); the records are the
 * payload d_payload (word 0 = count, as pbd_detect_batch_device_out leaves it): min(max(word 0, 0), capacity) records are
 * read, so a -1 payload (a suppression overflow) writes nothing; d_out = double[6 * capacity] on the device.  Asynchronous on
 * pbd_stream().  A record whose frame index is out of range or whose nparts is outside 1..max parts gets six NaNs.
 * Neither call touches the resident detect result (pbd_get_stage, pbd_argmin_device_out read it as before). */
struct pbd_frame;   /* defined with pbd_detect_frames below */
int pbd_boxes3d(pbd_handle *h, int nframes, const struct pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                const int32_t *cand, int ncand, int frame_offset, double *out);
int pbd_boxes3d_device(pbd_handle *h, int nframes, const struct pbd_frame *d_depth, int depth_code, const int *im_rows,
                       const int *im_cols, const int32_t *d_payload, int capacity, int frame_offset, double *d_out);

/* Camera boxes and part centres (new surface; opt-in): the rest of PointCloudClusterer::computeBoundingBoxes
 * (include/PointCloudClusterer.hpp:53-153; cells/detect.cpp:224-275, ros/Node.cpp:183-230).
 * Pinhole model, this library's contract: ray(u, v) = (((u - cx) - tx) / fx, ((v - cy) - ty) / fy, 1.0) in double, which is
 * image_geometry's PinholeCameraModel::projectPixelTo3dRay as the ROS node binds it (ros/Node.cpp:210).  The ECTO cell's
 * image_pipeline projector (cells/detect.cpp:193-200) is not pinned.  One pbd_pinhole per frame; a non-finite or zero fx / fy
 * is PBD_ERR_INVALID naming the frame.
 * Per record (frame index = frame - frame_offset, as pbd_boxes3d), in double unless said otherwise:
 *   cube     what pbd_boxes3d computes for the record.  A NaN in any of its six values skips the record (the reference's
 *            `continue`): camera box {0,0,0,0,0,0}, ncentres 0, dense 1
 *   box      tl = ray(cube.x, cube.y) * cube.z, br = ray(cube.x + cube.width, cube.y + cube.height) * (cube.z + cube.depth);
 *            out = Rect3d(tl, br) = {tl.x, tl.y, tl.z, br.y - tl.y, br.x - tl.x, br.z - tl.z} (Rect3d member order)
 *   centres  part j: part &= Rect(0, 0, im_cols, im_rows) (empty -> Rect()); centre pixel (x + w/2, y + h/2), int division;
 *            avg = double sum of the float depth samples in row-major order, / (w*h) when w*h != 0; the point is
 *            ray(centre) * avg with each component rounded to float (pcl::PointXYZ).  An empty part gives ray(0,0) * 0.0
 *            (signed zeros).  dense = 0 when any component of any centre is NaN; ncentres = nparts
 *   samples  PBD_PARTS_LITERAL (the default, a reference quirk kept as the Iy composition quirk is): rows x .. x+h-1, columns
 *            y .. y+w-1, the reference's transposed loop (:111-120).  PBD_PARTS_XY: rows y .. y+h-1, columns x .. x+w-1, the box
 *            in its own orientation.  Project decision: a non-empty part whose sample rectangle leaves the depth image (the
 *            reference reads outside it, undefined behaviour) has the centre {NaN, NaN, NaN}
 * The depth images must be 32F (depth_code 5, what the reference reads, :113); any other code is PBD_ERR_UNSUPPORTED.
 * Outputs: box double[6*n], centres float[3*max_parts*n] (record i, part j at 3*(i*max_parts + j)), ncentres int32[n], dense
 * int32[n].  pbd_boxes3d_camera: host records / images / outputs, synchronous; centres past ncentres are 0.
 * pbd_boxes3d_camera_device: the payload and depth frames as pbd_boxes3d_device, device outputs of `capacity` records, only the
 * min(max(word 0, 0), capacity) records written (centres past ncentres untouched); asynchronous on pbd_stream().
 * Validation, PBD_ERR_STATE and the resident result as pbd_boxes3d. */
typedef struct pbd_pinhole { double fx, fy, cx, cy, tx, ty; } pbd_pinhole;
enum { PBD_PARTS_LITERAL = 0, PBD_PARTS_XY = 1 };
int pbd_boxes3d_camera(pbd_handle *h, int nframes, const struct pbd_frame *depth, int depth_code, const int *im_rows,
                       const int *im_cols, const pbd_pinhole *cams, int parts_mode, const int32_t *cand, int ncand, int frame_offset,
                       double *box, float *centres, int32_t *ncentres, int32_t *dense);
int pbd_boxes3d_camera_device(pbd_handle *h, int nframes, const struct pbd_frame *d_depth, int depth_code, const int *im_rows,
                              const int *im_cols, const pbd_pinhole *cams, int parts_mode, const int32_t *d_payload, int capacity,
                              int frame_offset, double *d_box, float *d_centres, int32_t *d_ncentres, int32_t *d_dense);

/* Object clusters (new surface; opt-in): PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:157-293).
 * With plane removal (organizedMultiplaneSegmentation, off by default at ros/Node.hpp:145) the caller passes the reduced,
 * unorganized cloud pbd_remove_planes* writes (below); the indices then refer to that cloud, as in the reference.
 * pbd_cloud: x, y, z are the first three floats of every point (a pcl::PointXYZ / PointXYZRGB buffer as it is); point (r, c)
 * at data + r * row_stride + c * point_stride, index r * cols + c; rows == 1 is an unorganized cloud.  Refused
 * (PBD_ERR_INVALID, naming the cloud): a non-positive size, rows * cols >= 2^31, point_stride < 12, row_stride below the
 * row's bytes (rows > 1), and on the device a pointer or stride not a multiple of 4.
 * Per box (camera boxes as pbd_boxes3d_camera writes them; frame = the box's cloud):
 *   gate     volume = width * height * depth; if volume >= 1e-6: x -= width * 0.1 (y, z likewise), width *= 1.2 (height,
 *            depth likewise); min = (float)(x, y, z), max = (float)(x + width, y + height, z + depth).  Otherwise no points
 *   crop     pcl::CropBox on a cloud taken as not dense: the finite points with min <= p <= max on all three axes, in float,
 *            in ascending index order
 *   edges    library definition (PCL's organized / kd-tree boundary convention is not pinned): two cropped points are
 *            neighbours iff (double)d2 <= (double)0.01f * (double)0.01f, d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, each
 *            operation rounded separately
 *   cluster  the connected components (min size 1); the largest is kept.  Project decision: on a size tie the one whose
 *            smallest point index is lowest (the reference leaves ties to an unstable std::sort, :253-260)
 *   centre   pcl::compute3DCentroid: three fp32 sums in ascending index order, each / (float)count; NaN x3 without a cluster
 *   output   centres float[3*n]; counts int32[n] (the kept cluster's size, 0 without one); indices: the kept clusters' point
 *            indices in ascending order, box after box (the caller gathers the points, as ExtractIndices copies them)
 * pbd_cluster_objects: host clouds, boxes double[6*nboxes] and frames[nboxes] (cloud index; outside 0..nclouds-1 is
 * PBD_ERR_INVALID naming the box); synchronous.  *needed = the total of counts; when it exceeds index_capacity:
 * PBD_ERR_CAPACITY and no output is written.  More than 2^29 cropped points in one call: PBD_ERR_INVALID.
 * pbd_cluster_objects_device: device clouds (a region of a larger buffer is read in place), the boxes' frames from the payload
 * (box i's frame = record i's frame - frame_offset; min(max(word 0, 0), capacity) boxes; a frame outside 0..nclouds-1: no
 * points), d_boxes double[6*capacity].  crop_capacity bounds the cropped points of all boxes together (at most 2^29, above
 * that PBD_ERR_INVALID; the handle's workspace, about 52 bytes per point, grows to it), index_capacity the output indices.  d_status int64[2] = {cropped points, output indices}; status[1] is -1
 * when the crop overflowed, and then every box has count 0 and a NaN centre; when status[1] > index_capacity the indices are
 * not written.  Nothing is written out of bounds.  Asynchronous on pbd_stream(), no host synchronisation.
 * PBD_ERR_STATE while a batch is in flight; the resident detect result is not touched. */
typedef struct pbd_cloud {
    const void *data;
    int rows, cols;
    size_t point_stride, row_stride;
} pbd_cloud;
int pbd_cluster_objects(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const double *boxes, const int *frames, int nboxes,
                        float *centres, int32_t *counts, int32_t *indices, int index_capacity, int *needed);
int pbd_cluster_objects_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const int32_t *d_payload, int capacity,
                               int frame_offset, const double *d_boxes, int crop_capacity, int index_capacity, float *d_centres,
                               int32_t *d_counts, int32_t *d_indices, long long *d_status);

/* Plane removal (new surface; opt-in): PointCloudClusterer::organizedMultiplaneSegmentation (include/PointCloudClusterer.hpp:
 * 294-336): IntegralImageNormalEstimation (AVERAGE_3D_GRADIENT), OrganizedMultiPlaneSegmentation::segmentAndRefine, and
 * ExtractIndices(negative) of every plane's inliers.  PCL is not pinned: this is the library's own restatement of the algorithm
 * with the reference's parameters, and every deviation is named here.  P(r, c) is the point at row r, column c of an organized
 * pbd_cloud, z its third coordinate; a point is finite when x, y and z are.  Every float / double operation below is rounded
 * on its own, in the order written (no contraction).  s = smoothing_size / 2.
 *   normals  dx(r,c) = P(r,c+1) - P(r,c-1), dy(r,c) = P(r+1,c) - P(r-1,c) in fp32.  Depth edge: a pixel not finite, or with a
 *            4-neighbour q not finite or |z(q) - z(p)| > depth_change_factor * z(p).  The window is rows r-s..r+s, columns
 *            c-s..c+s.  Project decision: the normal is NaN unless s+1 <= r <= rows-s-2 and s+1 <= c <= cols-s-2 (the window and
 *            the one-pixel ring its gradients read lie in the image; PCL shrinks the window near the border instead) and no
 *            window pixel is a depth edge.  Otherwise: each window row summed left to right from 0, those row sums summed top to
 *            bottom from 0, each / (float)((2s+1)^2) -> mx (from dx), my (from dy); n = cross(my, mx) = (my.y*mx.z - my.z*mx.y,
 *            my.z*mx.x - my.x*mx.z, my.x*mx.y - my.y*mx.x); n /= sqrt((n.x*n.x + n.y*n.y) + n.z*n.z) (three divides); if
 *            (n.x*P.x + n.y*P.y) + n.z*P.z > 0 then n = -n.  d(p) = (n.x*P.x + n.y*P.y) + n.z*P.z after the flip
 *   segments p is joined to its left and its upper neighbour q when q is finite, |d(p) - d(q)| < distance_threshold * (z(p)*z(p))
 *            (PlaneCoefficientComparator, depth dependent, the current point's z) and (n(p).x*n(q).x + n(p).y*n(q).y) +
 *            n(p).z*n(q).z > (float)cos(angular_threshold).  A NaN normal fails; a point that is not finite is in no segment.
 *            Segments are the connected components, numbered by their smallest point index
 *   planes   a segment of more than min_inliers points whose curvature is below max_curvature, in segment order.  Moments
 *            {x, y, z, xx, xy, xz, yy, yz, zz} in double ((double)x * (double)y): per image row the segment's points left to
 *            right from 0, those row partials top to bottom from 0; mean m = sum / count; covariance c_ij = m_ij - m_i * m_j.
 *            Smallest eigenpair: 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) from V = I (a pair with a_pq == 0 is skipped;
 *            theta = (a_qq - a_pp) / (2 a_pq), t = 1 / (|theta| + sqrt(theta*theta + 1)) negated when theta < 0,
 *            c = 1 / sqrt(t*t + 1), s = t*c; A <- J^T (A J), V <- V J, each updated column / row entry c*u - s*v and s*u + c*v);
 *            lambda = the smallest diagonal entry (the first on a tie), its column of V the eigenvector (a, b, c), no other sign
 *            convention.  curvature = lambda / ((c_xx + c_yy) + c_zz).  d = -((a*m_x + b*m_y) + c*m_z); all four negated when
 *            ((-m_x)*a + (-m_y)*b) + (-m_z)*c < 0; rounded to float (pcl::ModelCoefficients)
 *   refine   (refine = 1; PCL's refine, two in-place raster passes of the label image with PlaneRefinementComparator).  Forward:
 *            rows 0..rows-2 top to bottom, columns 0..cols-2 left to right; at each current cell the right neighbour, then the
 *            lower one; `continue` when the current or the right label is negative, and before the lower check when the lower
 *            label is.  Backward: the same on the image turned by 180 degrees (rows rows-1..1, columns cols-1..1, left then
 *            upper neighbour).  Project decision: the backward columns stop at 1 (column 0 has no left neighbour).  A neighbour is
 *            absorbed when the current label is a plane's segment, the neighbour's is not, and
 *            |((a*x + b*y) + c*z) + d| < distance_threshold * (z(current)*z(current)) on the neighbour's point in fp32; it takes
 *            the plane's label and may absorb cells later in the pass.  As a recurrence in a pass's own coordinates (o = the
 *            labels at the pass's start; whether a label is negative never changes, so the right label's test reads o):
 *              M(r,c) = F(r-1,c) if r >= 1, c <= cols-2, F(r-1,c) is a plane, o(r-1,c+1) >= 0, o(r,c) >= 0 is no plane and
 *                       P(r,c) is absorbed with z(r-1,c); else o(r,c)
 *              F(r,c) = F(r,c-1) if c >= 1, r <= rows-2, F(r,c-1) is a plane, M(r,c) >= 0 is no plane and P(r,c) is absorbed
 *                       with z(r,c-1); else M(r,c)
 *            so a pass is a wavefront over the anti-diagonals r + c
 *   output   removed = every point whose final label is a plane.  The reduced cloud: every other point, NaN points included, as
 *            xyz float triples in ascending index order (ExtractIndices, negative): an unorganized cloud
 * Parameters: pbd_plane_params; NULL is the reference's call (smoothing 10, depth change 0.02, distance 0.02, angle 3 degrees =
 * 3.0 * M_PI / 180.0, curvature 0.001, min inliers 1000, refine 1).  refine = 0 is segment() alone.
 * Outputs, cloud i of n_i = rows * cols points at base_i = n_0 + ... + n_(i-1) of the point-indexed arrays:
 *   points   float[3 * total]: the reduced cloud (nkept[i] points) at 3 * base_i, then NaN points up to n_i: {points + 3 * base_i,
 *            rows 1, cols n_i, point_stride 12, row_stride 12 * n_i} is a pbd_cloud pbd_cluster_objects* read as it is (a NaN
 *            point is never cropped); kept int32[total]: the kept points' original indices, then -1; nkept int32[nclouds];
 *   labels   int32[total]: the plane's index, or -1
 *   planes   float[4 * plane_capacity * nclouds] (cloud i, plane k at 4 * (i * plane_capacity + k)): a, b, c, d; inliers
 *            int32[plane_capacity * nclouds] after refinement; nplanes int32[nclouds]
 * Refused (PBD_ERR_INVALID, naming the cloud): rows < 2 or cols < 2, the pbd_cloud rules above, 2^31 or more points in one call;
 * and parameters outside smoothing 2..128, min_inliers >= 0, refine 0 / 1, finite thresholds.
 * pbd_remove_planes: host clouds and outputs, synchronous; *needed = the most planes of one cloud; above plane_capacity:
 * PBD_ERR_CAPACITY and no output is written.
 * pbd_remove_planes_device: device clouds (a region of a larger buffer is read in place), device outputs; d_status int64[2] =
 * {kept points of all clouds, the most planes of one cloud}; nplanes[i] may exceed plane_capacity, and then only the first
 * plane_capacity planes of the cloud are written (labels still name every plane).  Asynchronous on pbd_stream(), no host
 * synchronisation; the handle's workspace (about 80 bytes per point) grows to the call.
 * PBD_ERR_STATE while a batch is in flight; the resident detect result is not touched. */
typedef struct pbd_plane_params {
    int smoothing_size;          /* 10: the window half size is smoothing_size / 2 */
    float depth_change_factor;   /* 0.02 */
    float distance_threshold;    /* 0.02 (the comparators' and the refinement's) */
    double angular_threshold;    /* radians, 3 degrees; the comparator uses (float)cos(angular_threshold) */
    double max_curvature;        /* 0.001 */
    int min_inliers;             /* 1000: a plane has more points than this */
    int refine;                  /* 1: segmentAndRefine, 0: segment */
} pbd_plane_params;
int pbd_remove_planes(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const pbd_plane_params *params, float *points,
                      int32_t *kept, int32_t *nkept, int32_t *labels, float *planes, int32_t *inliers, int32_t *nplanes,
                      int plane_capacity, int *needed);
int pbd_remove_planes_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const pbd_plane_params *params, float *d_points,
                             int32_t *d_kept, int32_t *d_nkept, int32_t *d_labels, float *d_planes, int32_t *d_inliers,
                             int32_t *d_nplanes, int plane_capacity, long long *d_status);

/* Depth consistency (new surface; opt-in): SearchSpacePruning<T>::filterCandidatesByDepth(parts, candidates, depth, zfactor)
 * (src/SearchSpacePruning.cpp:73-95), the step detect(im, depth) documents ("used for depth consistency and search space
 * pruning", src/PartsBasedDetector.cpp:65) and leaves commented out (:91-93, zfactor 0.03).  It runs before the callers' sort and
 * suppression: chain it with pbd_suppress* below.  Records are this handle's, unsuppressed (pbd_set_nms off); a record's frame index
 * is its `frame` field minus frame_offset, as pbd_boxes3d; the model tables are the handle's.  T is the handle's real type.
 * depth[f]: frame f's depth image, one channel, depth_code 0 (8U), 2 (16U), 5 (32F) or 6 (64F), one code per call, any pitch.
 *   samples  part j's box (x, y, w, h of component-local part j of the record) in the depth image's own coordinates, unscaled (as
 *            the reference reads depth(child)), & Rect(0, 0, dcols, drows) in 64-bit arithmetic.  Project decision: the reference's
 *            ROI throws cv::Exception for a box that leaves the image.  Every pixel of the clipped box is one sample, zeros
 *            included, converted to T (8U / 16U exactly, 64F to float rounded to nearest).  Project decision: a NaN sample reads as
 *            0 (ROS depth marks "no reading" with NaN; std::nth_element over NaN is undefined)
 *   median   M = the clipped area; the sample at 0-based index M / 2 of the samples sorted ascending (nth_element(first, first +
 *            M/2, last): the upper median for even M), exact; -0.0 == +0.0.  An empty clipped box has no median
 *   edges    for p = 1 .. nparts-1, q = parentid[c][p] (component-local), mc / mq the medians of parts p / q: the record is
 *            rejected when both exist, mc > 0, mq > 0 and (double)std::abs(mc - mq) > std::sqrt((double)ax*ax + (double)ay*ay) *
 *            (double)zfactor, the subtraction and abs in T, (ax, ay) = anchors[defid[mix_offset[gp] + 0]] (part.anchor(0), the
 *            mixture-0 anchor).  A NaN difference (Inf - Inf) does not reject.  The order of the edges does not matter (the
 *            reference's `break` is an optimisation)
 *   one part project decision: a record of a one-part component is kept (the reference's `size_t p = nparts-1; p >= 1` loop drops
 *            every such record, a defect)
 *   output   the kept records in input order (a stable compaction), byte-identical to their input, `frame` fields unchanged
 * pbd_depth_consistency: host records and images, synchronous.  *nout = the kept count; above `capacity` the first `capacity`
 * records are written and the call returns PBD_ERR_CAPACITY.  out == cand (in place) is allowed.
 * pbd_depth_consistency_device: d_depth[f].data are device pointers (a frame may be a region of a larger image, read in place);
 * the records are the payload d_payload (word 0 = count, capacity records); d_out = int32[1 + out_capacity * stride]: word 0 = the
 * kept count, which may exceed out_capacity (then the first out_capacity records are written).  An input word 0 that is negative
 * (a suppression overflow) or > capacity (a truncated list) gives word 0 = -1 and no records: a filtered truncated list is never
 * mistaken for a complete one.  A record whose frame index is out of range, whose component is unknown or whose nparts is not its
 * component's part count (1..max parts) is dropped.  d_out must not overlap d_payload.  Asynchronous on pbd_stream(), no host
 * synchronisation; the handle's workspace grows with capacity (about 12 bytes per part of a record), never with the samples.
 * Refused with PBD_ERR_INVALID, naming the index, before anything is enqueued: a depth_code other than the four, a non-positive
 * size, an image of 2^31 pixels or more, a pitch below the row bytes, on the device a pointer or pitch not a multiple of the
 * element size; in the host form a record whose frame index, component or nparts is bad as above; a NaN zfactor (any other
 * zfactor, infinities included, is taken as given).  PBD_ERR_STATE while a batch is in flight.  The resident detect result is not
 * touched. */
int pbd_depth_consistency(pbd_handle *h, int nframes, const struct pbd_frame *depth, int depth_code, float zfactor,
                          const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity, int *nout);
int pbd_depth_consistency_device(pbd_handle *h, int nframes, const struct pbd_frame *d_depth, int depth_code, float zfactor,
                                 const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity);

/* Scale-depth pruning of roots (new surface; opt-in): the intent of SearchSpacePruning<T>::filterResponseByDepth
 * (src/SearchSpacePruning.cpp:47-70), the other step detect(im, depth) leaves commented out (src/PartsBasedDetector.cpp:86-93).  The
 * stub is unfinished; its comments ask for "a mask of plausible depths given the object size and the scale of the image" and it
 * computes Z = fx * X / scales[n].  The arithmetic below is the project's decision, stated here once:
 *   plausible(rect, depth, fx, width, tol) -> bool
 *   rect   (x, y, w, h), the root part's rectangle of a record: words 8..11, what the walk writes for part 0
 *   depth  the frame's depth image: one channel, depth_code 0 (8U), 2 (16U), 5 (32F) or 6 (64F), any pitch, the SAME rows x cols
 *          as the colour frame of the record
 *   fx     focal length in pixels; width: the physical width of the root filter's footprint in the depth image's units; tol: a
 *          relative tolerance.  All float, widened to double.  fx and width finite and > 0, tol finite and >= 0; anything else is
 *          PBD_ERR_INVALID
 *   1. w <= 0: true.
 *   2. x1 = max(x, 0), y1 = max(y, 0), x2 = min(x + w, cols), y2 = min(y + h, rows) (64-bit); x2 - x1 <= 0 or y2 - y1 <= 0: true.
 *   3. nine samples, i, j in {0, 1, 2}: px_i = x1 + ((2 i + 1) * (x2 - x1)) / 6, py_j = y1 + ((2 j + 1) * (y2 - y1)) / 6 (integer
 *      division), d = (double)depth[py_j][px_i]; a sample is valid when d > 0 && d < +inf (NaN, zeros, negatives and Inf are holes).
 *   4. Z = ((double)fx * (double)width) / (double)w -- w the rectangle's own width, not the clipped one.
 *   5. a valid sample is in band when fabs(d - Z) <= (double)tol * Z, in double, no contraction.
 *   6. true when no sample is valid (unknown depth never prunes) or any valid sample is in band; false otherwise.
 * The result does not depend on the handle's T.
 * pbd_set_depth_prune(h, cfg): cfg = NULL turns it off (the default).  Kept across model updates; PBD_ERR_STATE while a batch is in
 * flight (the setting is latched at submit); the resident result stays.
 * pbd_bind_depth / pbd_bind_depth_device: attach the depth images of the NEXT call of any entry point pbd_set_root_nms lists, or
 * of pbd_argmin_device_out (which so re-emits the resident list under another depth or other parameters without running the dynamic
 * program again).  That call consumes the binding.  With pruning on, it first writes a byte per root cell -- above the threshold
 * and plausible, the rectangle built from the cell, the root mixture's filter size and the level's scale exactly as the walk would
 * -- and the find additionally requires the byte: the same records, fewer of them, in the same order.  With pbd_set_root_nms on as
 * well, the grid maxima are taken among the plausible cells above the threshold only.  max_candidates, the caller's capacity,
 * PBD_ERR_CAPACITY, payload word 0 and pbd_set_nms see only the kept list.  Level sharding is allowed (the test is per cell).
 *   nframes == 0 unbinds.  Pruning on and nothing bound: no pruning, as detect(im) without depth.  Bound and pruning off: the
 *   binding is dropped unused.  If the binding's nframes or a frame's rows x cols differ from the call's frames, the call returns
 *   PBD_ERR_INVALID naming the frame, nothing is enqueued and the binding is dropped.
 *   The host form copies the images now, into a buffer of the handle (on pbd_stream(), behind the work already queued).  The device
 *   form reads them in place: they must stay valid until the call's work has run (until _wait for the pipelined form); a frame may
 *   be a region of a larger image.  Both may be called while a batch is in flight.  Refusals as pbd_depth_consistency*'s images.
 *   NOT applied by pbd_dp_argmin, pbd_detect_latent, or the trainers' re-walks, for the reason root NMS is not.
 * pbd_depth_prune / pbd_depth_prune_device: the same decision per record of a caller's list, the rectangle taken from the record
 * (no model and no scales are read).  Conventions of pbd_depth_consistency* above, word for word: frame_offset, in place allowed
 * for the host form, *nout / word 0 = the kept count (which may exceed the capacity), an input word 0 that is negative or > capacity
 * gives -1, a record whose frame index is out of range or whose nparts is outside 1..max parts is dropped (host form: refused), no
 * host synchronisation in the device form, the resident result untouched, PBD_ERR_STATE while a batch is in flight.
 * pbd_set_depth_prune(h, cfg != NULL) on a handle with a non-zero pbd_set_padding is PBD_ERR_UNSUPPORTED, as is a non-zero padding
 * while the pruning is enabled: the rule has no padded form yet. */
typedef struct pbd_depth_prune_cfg { float fx, width, tol; } pbd_depth_prune_cfg;
int pbd_set_depth_prune(pbd_handle *h, const pbd_depth_prune_cfg *cfg);
int pbd_bind_depth(pbd_handle *h, int nframes, const struct pbd_frame *depth, int depth_code);
int pbd_bind_depth_device(pbd_handle *h, int nframes, const struct pbd_frame *d_depth, int depth_code);
int pbd_depth_prune(pbd_handle *h, const pbd_depth_prune_cfg *cfg, int nframes, const struct pbd_frame *depth, int depth_code,
                    const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity, int *nout);
int pbd_depth_prune_device(pbd_handle *h, const pbd_depth_prune_cfg *cfg, int nframes, const struct pbd_frame *d_depth, int depth_code,
                           const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity);

/* The K best of every segment (new surface; opt-in).  The rule, stated here once:
 *   order        a is BETTER than b when value(a) > value(b), compared as numbers in the array's own type; if the values are equal, a
 *                is better when its element index is smaller.  +0.0 and -0.0 tie; +Inf ties +Inf.
 *   eligible     an element that is not NaN and, where a mask is given, whose mask byte is non-zero
 *   selection    of each segment -- a contiguous range of elements -- the min(K, eligible) best eligible elements are kept and
 *                nothing else.  The order is total, so the kept set is unique.
 * pbd_top_k_cells / pbd_top_k_cells_device: nseg segments packed back to back, segment i of len[i] elements (a host array in both
 * forms; 0 is legal); `mask` (NULL: none) and `dst` have the same layout; dst receives 0 or 255 in every byte.  real_code is
 * PBD_REAL_F32 or PBD_REAL_F64, whatever the handle's T: the handle gives the stream, the workspace and the error text only.
 * k >= 0; k == 0 keeps nothing.  PBD_ERR_INVALID: a negative k, nseg or len, a total above 2^31 - 1, another real_code, or NULL
 * src / dst / len with work to do.  PBD_ERR_STATE while a batch is in flight.  The resident detect result is not touched.
 * The host form is synchronous; the device form (d_src aligned to its element) is asynchronous on pbd_stream().  Two calls on the
 * same input give the same bytes, and the cost does not depend on the values.
 * pbd_set_top_k(h, k): k == 0 is off (the default on a new handle), 1 .. 2^30 on, anything else PBD_ERR_INVALID; PBD_ERR_STATE while
 * a batch is in flight (the setting is latched at submit).  Kept across model updates; the resident result stays.  With it on, every
 * later call of the entry points pbd_set_root_nms lists, and pbd_argmin_device_out (which so re-emits the resident list under
 * another K without running the dynamic program again), runs the selection over rootv in the handle's T with one segment per frame:
 * frame f of an equal-size batch is the root cells [f * cells * NC, (f + 1) * cells * NC) (cells: the root cells of one frame's
 * levels), a frame of a mixed-size call the range of its own levels.  Eligible means `rootv > (T)thresh`, the find's own expression,
 * and the byte of depth pruning and of root NMS where those are on: K is taken among the survivors of both.  The find additionally
 * requires the new byte.  Result: the same records, fewer of them -- at most K per frame whatever the threshold and the scene --
 * in the same (frame, level, component, y, x) order; every word of a kept record is untouched.  max_candidates, the caller's
 * capacity, PBD_ERR_CAPACITY, payload word 0 and pbd_set_nms see only the kept list.  NOT applied by pbd_dp_argmin,
 * pbd_detect_latent, or the trainers' re-walks, for the reason root NMS is not.  Level sharding is allowed: each rank keeps the K
 * best of its own levels, so the union over the ranks contains the unsharded result, and pbd_top_k on the merged list put in
 * (frame, level, component, y, x) order IS the unsharded result for T = float.  For T = double the records carry a float score, so
 * only the detect-path form sees differences below float precision.
 * pbd_top_k / pbd_top_k_device: per frame of a caller's list, the K best records by the record's float score (k >= 0, else
 * PBD_ERR_INVALID).  A record with a NaN score is never kept, as the find never lists one; ties go to the earlier record of the
 * list; the kept records come out in their input order.  Records must be grouped by ascending frame, as for pbd_suppress* (host
 * form: refused otherwise).  Conventions of pbd_depth_prune* above, word for word: frame_offset, in place allowed for the host form,
 * *nout / word 0 = the kept count (which may exceed the capacity), an input word 0 that is negative or > capacity gives -1, a record
 * whose frame index is outside 0 .. nframes - 1 or whose nparts is outside 1..max parts is dropped and is nobody's rival (host form:
 * refused), no host synchronisation in the device form, the resident result untouched, PBD_ERR_STATE while a batch is in flight. */
int pbd_top_k_cells(pbd_handle *h, int nseg, const long long *len, int real_code, const void *src, const uint8_t *mask, int k,
                    uint8_t *dst);
int pbd_top_k_cells_device(pbd_handle *h, int nseg, const long long *len, int real_code, const void *d_src, const uint8_t *d_mask,
                           int k, uint8_t *d_dst);
int pbd_set_top_k(pbd_handle *h, int k);
int pbd_top_k(pbd_handle *h, int nframes, int k, const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity,
              int *nout);
int pbd_top_k_device(pbd_handle *h, int nframes, int k, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out,
                     int out_capacity);

/* Scale NMS: a root's duplicates on neighbouring pyramid levels and components (new surface; opt-in, off on a new handle).  An
 * object fires at the same image position on several neighbouring levels and on several components; root NMS works inside one
 * (level, component) plane only.  The reference's commented-out call took the scales: ssp_.nonMaxSuppression(rootv, scales)
 * (src/PartsBasedDetector.cpp:86).  The rule, stated here once; all arithmetic is integer, on the rectangle the walk writes:
 *   rect(r)          (x, y, w, h), the rectangle of part 0 of root r: words 8..11 of its record.  For a root cell: part_rect of the
 *                    cell with the winning root type's filter side, the level's scale and the pad of pbd_set_padding
 *   covers(a, b)     w_a > 0 and h_a > 0 and 2 x_a <= 2 x_b + w_b < 2 (x_a + w_a) and 2 y_a <= 2 y_b + h_b < 2 (y_a + h_a): b's
 *                    centre, doubled to stay in integers, lies inside a's rectangle
 *   neighbours(a, b) a != b, both in the same frame, |level_a - level_b| <= dl, and covers(a, b) or covers(b, a).  Symmetric.
 *                    Every component takes part, and a's own plane does.  Levels are the indices of the frame's own level list
 *                    (with the fine octave the longer list, whose scales still ascend; in a mixed-size or region call the frame's
 *                    own levels); dl at or above the level count means every level
 *   better(a, b)     score_a > score_b; at equal scores (+0.0 and -0.0 tie) a is better when it comes earlier in the find order
 *                    (level, component, y, x).  The order is total.  In the detect path the scores are rootv in the handle's T; in
 *                    the list form the records' float scores, and earlier means earlier in the list -- pbd_top_k*'s conventions,
 *                    its remark on T = double included: only the detect-path form sees differences below float precision
 *   eligible         rootv > (T)thresh, the find's own expression (NaN never is), and the bytes of depth pruning and of root NMS
 *                    where those are on: the step runs after both and before top-K
 *   result           an eligible root is kept iff no eligible neighbour is better.  A local-maximum rule, not a greedy pass: a
 *                    root a better neighbour beats is dropped even if that neighbour is dropped itself.  The result does not
 *                    depend on the order of evaluation; of two neighbouring roots at most one survives; a frame's best root does
 * pbd_set_scale_nms(h, enable, dl): dl in 0..255 whatever `enable`, else PBD_ERR_INVALID; enable = 0 is off.  PBD_ERR_STATE while a
 * batch is in flight (the setting is latched at submit); kept across model updates; the resident result stays.  With it on, every
 * later call of the entry points pbd_set_top_k lists -- pbd_argmin_device_out included, which so re-emits the resident list
 * under another dl without running the dynamic program again -- keeps only the scale-space maxima: the same records, fewer of
 * them, in the same order, every word untouched.  max_candidates, the caller's capacity, PBD_ERR_CAPACITY, payload word 0,
 * pbd_set_top_k (K is taken among the maxima) and pbd_set_nms see only the kept list.  NOT applied by pbd_dp_argmin,
 * pbd_detect_latent* or the trainers' re-walks.  PBD_ERR_UNSUPPORTED together with level sharding (world > 1), in either order of
 * the two calls, as for pbd_set_nms: one rank does not hold the neighbouring levels; pbd_scale_nms on the merged list is the form
 * for sharded handles.
 * pbd_scale_nms / pbd_scale_nms_device: the rule per frame of a caller's list (dl in 0..255, else PBD_ERR_INVALID).  A record with a
 * NaN score is never kept and is nobody's neighbour; the kept records come out in their input order.  Records must be grouped by
 * ascending frame, as for pbd_suppress* (host form: refused otherwise).  Conventions of pbd_depth_prune* above, word for word:
 * frame_offset, in place allowed for the host form, *nout / word 0 = the kept count (which may exceed the capacity), an input word 0
 * that is negative or > capacity gives -1, a record whose frame index is outside 0 .. nframes - 1 or whose nparts is outside
 * 1..max parts is dropped and is nobody's rival (host form: refused), no host synchronisation in the device form, the resident
 * result untouched, PBD_ERR_STATE while a batch is in flight.  Each record tests the records of its frame: the cost grows with
 * the square of a frame's list. */
int pbd_set_scale_nms(pbd_handle *h, int enable, int dl);
int pbd_scale_nms(pbd_handle *h, int nframes, int dl, const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity,
                  int *nout);
int pbd_scale_nms_device(pbd_handle *h, int nframes, int dl, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out,
                         int out_capacity);

/* Suppression of a caller's list (new surface): exactly the pbd_set_nms stage above -- per frame the stable score sort, then the
 * greedy painted-canvas suppression -- applied to any records of this handle, e.g. after pbd_depth_consistency, or to the merged
 * lists of level-sharded handles (pbd_set_nms itself stays refused with sharding: one rank's levels are not the union).
 * A record's frame is `frame` - frame_offset and has its own Rect(0, 0, im_cols[f], im_rows[f]) (1..65536 each).  Records must
 * be grouped by ascending frame.  Output: frame by frame, each frame's kept records in sorted order, `frame` fields unchanged.
 * pbd_suppress: host records, synchronous; a record whose frame index is out of range, lower than its predecessor's, or whose
 * nparts is outside 1..max parts is PBD_ERR_INVALID naming the record; *nout = the kept count, above `capacity` the first `capacity`
 * records and PBD_ERR_CAPACITY.  In place (out == cand) is allowed.
 * pbd_suppress_device: the payload and output as pbd_depth_consistency_device (word 0 = kept count, may exceed out_capacity; an
 * input word 0 that is negative or > capacity gives -1).  Project decision: a device list with a frame index out of range or not
 * grouped ascending also gives word 0 = -1.  capacity must be at least 1 (PBD_ERR_INVALID otherwise; out_capacity may be 0).
 * Asynchronous on pbd_stream() while the list of frame sizes is that of the previous pbd_suppress* call; a new list of frame
 * sizes synchronises the stream and uploads its small canvas tables first (both forms).  A NaN overlap or a bad size is
 * PBD_ERR_INVALID; PBD_ERR_STATE while a batch is in flight;
 * the resident detect result is not touched. */
int pbd_suppress(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap,
                 const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity, int *nout);
int pbd_suppress_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap,
                        const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity);

/* ---- Testing a model (new surface; opt-in): the reference's Matlab test code on the device -- matlab/detection/testmodel.m,
 * testmodel_gtbox.m, nms.m, bestoverlap.m and matlab/evaluation/eval_pck.m, eval_apk.m, VOCap.m.  DESIGN.md section 6l.
 * Shared by the four calls:
 *   records  this handle's (pbd_candidate_stride); a record's frame is its `frame` field - frame_offset.  Every record is read
 *            with the model's part count nparts; a model whose components differ in part count is PBD_ERR_UNSUPPORTED (Matlab's
 *            box matrix has one width).  The _device forms read min(max(word 0, 0), capacity) records of a payload, are
 *            asynchronous on pbd_stream() and take the ground truth from HOST arrays, as frame sizes are elsewhere
 *   corners  of part j: x1 = x, y1 = y, x2 = x + w, y2 = y + h, the two points the reference built the cv::Rect from
 *            (src/DynamicProgram.cpp:238-242): detect.m's corners rounded and shifted by one.  Areas are inclusive,
 *            (x2 - x1 + 1) * (y2 - y1 + 1), as in pbd_detect_latent.  Every formula depends on coordinate differences only, so
 *            0-based and 1-based coordinates give the same result.  Centre of part j: (.5 * x1 + .5 * x2, .5 * y1 + .5 * y2)
 *   numbers  all arithmetic is double, each operation rounded on its own in the order written, division and sqrt correctly
 *            rounded; min(a, b) is b < a ? b : a and max(a, b) is b > a ? b : a; no special cases beyond the ones stated (a
 *            record with a negative size follows IEEE)
 *   state    PBD_ERR_STATE while a batch is in flight; the resident detect result is not touched; nframes is 1..65535 and a
 *            list holds fewer than 2^30 parts (capacity * nparts), PBD_ERR_INVALID otherwise
 *
 * pbd_part_nms: nms.m per frame, the paper's suppression -- NOT the painted canvas of pbd_set_nms / pbd_suppress.  Records
 * grouped by ascending frame.  max_boxes is 1..1000 (Matlab's constant is 1000; PBD_ERR_INVALID otherwise).  Per frame:
 *   cut      with more than max_boxes records the list becomes its max_boxes highest scores in descending order, ties in list
 *            order (Matlab's stable sort(.., 'descend')); the list is reordered, as boxes(I(1:1000), :).  Otherwise it stays
 *   order    [vals, I] = sort(s) ascending and stable, taken from the end: the highest score first, among equal scores the LAST
 *            of the current list first; -0.0 and +0.0 tie
 *   boxes    b = 0 .. nparts of a record: its parts, then the hull min x1, min y1, max x2, max y2
 *   test     w = min(x2_i, x2_j) - max(x1_i, x1_j) + 1, 0 if negative, h likewise; o_b = (w * h) / area_i[b]; pick i removes
 *            every remaining j with max_b o_b > (double)overlap (a NaN o_b never does).  The divisor is the PICKER's area
 *   project decisions  the pick itself always leaves (Matlab loops forever when overlap >= 1); a NaN overlap is
 *            PBD_ERR_INVALID; NaN scores sort last, in list order, in the cut and in the pick order alike
 * Output as pbd_suppress*: frame by frame the kept records in pick order, unchanged.  pbd_part_nms: host records (a frame index
 * out of range or below its predecessor's, or nparts outside 1..max parts, is PBD_ERR_INVALID naming the record); *nout = the
 * kept count, above `capacity` the first `capacity` records and PBD_ERR_CAPACITY.  pbd_part_nms_device: d_out = int32[1 +
 * out_capacity * stride], word 0 = the kept count (may exceed out_capacity), or -1 for an input word 0 that is negative or above
 * capacity and for a list that is not grouped by ascending frame inside 0..nframes-1.  The workspace holds 128 KB per frame for
 * max_boxes = 1000 (a 1000 x 1000 bit matrix) plus 40 bytes per (frame, max_boxes) and 8 per record. */
int pbd_part_nms(pbd_handle *h, int nframes, float overlap, int max_boxes, const int32_t *cand, int ncand, int frame_offset,
                 int32_t *out, int capacity, int *nout);
int pbd_part_nms_device(pbd_handle *h, int nframes, float overlap, int max_boxes, const int32_t *d_payload, int capacity,
                        int frame_offset, int32_t *d_out, int out_capacity);
/* pbd_best_overlap: bestoverlap.m per frame, the step after detect_fast in testmodel_gtbox.m.  Records in any order.
 * gtbox = double[nframes][4] on the host, {x1, y1, x2, y2} inclusive; a NaN anywhere in a row: the frame has no ground truth
 * (Matlab's isempty(gtbox)).  A record passes when, with bx1 .. by2 the hull of its part CENTRES, w = min(x2, bx2) - max(x1, bx1)
 * + 1 (0 if negative), h likewise, (w * h) / gtarea > (double)overlap.  The passing record of the highest score wins, the FIRST
 * in list order among equals (Matlab's max); -0.0 and +0.0 tie.  Project decision: a record with a NaN score is never chosen.
 * Output as pbd_detect_latent: record f at out + f * stride and found[f]; a frame where nothing is found has found[f] = 0 and a
 * record of zeros.  The device form writes d_out and d_found, ignores records whose frame is out of range (the host form refuses
 * them) and takes lists of any length (the kernel strides over them).  A NaN overlap is PBD_ERR_INVALID. */
int pbd_best_overlap(pbd_handle *h, int nframes, const double *gtbox, float overlap, const int32_t *cand, int ncand, int frame_offset,
                     int32_t *out, int32_t *found);
int pbd_best_overlap_device(pbd_handle *h, int nframes, const double *gtbox, float overlap, const int32_t *d_payload, int capacity,
                            int frame_offset, int32_t *d_out, int32_t *d_found);
/* pbd_eval_pck: eval_pck.m on pbd_best_overlap's output: rec = int32[nframes][stride], found[nframes] (device pointers in the
 * device form), gt_points = double[nframes][nparts][2] and scale = double[nframes] on the host.  dist[p][f] = sqrt(dx * dx +
 * dy * dy) with d = centre - gt; a hit is dist < thresh * scale[f], strict; pck[p] = (double)hits / (double)nframes.  Project
 * decisions: a frame that is not found has dist = +Inf and is a miss; a NaN distance is a miss and is written as the quiet NaN
 * 0x7ff8000000000000 whatever its source.  Outputs pck[nparts] and, unless NULL,
 * dist[nparts][nframes].  Two quirks of the reference are NOT reproduced: its `nargin < 4` test always sets thresh = 0.5, and it
 * multiplies by the LAST frame's scale for every frame (a caller who wants that passes the last scale in every entry). */
int pbd_eval_pck(pbd_handle *h, int nframes, const int32_t *rec, const int32_t *found, const double *gt_points, const double *scale,
                 double thresh, double *pck, double *dist);
int pbd_eval_pck_device(pbd_handle *h, int nframes, const int32_t *d_rec, const int32_t *d_found, const double *gt_points,
                        const double *scale, double thresh, double *d_pck, double *d_dist);
/* pbd_eval_apk: eval_apk.m + VOCap.m for every part at once, on any list (typically pbd_part_nms's over a test set).  On the
 * host: gt_offset = int32[nframes + 1] (frame f's instances are gt_offset[f] .. gt_offset[f + 1] - 1; gt_offset[0] = 0,
 * non-decreasing), G = gt_offset[nframes], gt_points = double[G][nparts][2], gt_scale = double[G].  G == 0 is PBD_ERR_INVALID
 * (recall would be 0 / 0).  One order is shared by all parts: score descending, stable, NaN last.  Per part p and rank n of a
 * record of frame f: without ground truth in f the record is a false positive; otherwise d_g = sqrt(dx * dx + dy * dy) / scale_g
 * over the frame's instances, distmin the minimum and jmin its FIRST occurrence, NaN entries ignored (all NaN: a false positive);
 * the record is a true positive iff distmin <= thresh and no earlier rank of this frame with distmin <= thresh had the same jmin
 * (the gt.det flag).  rec[n] = tpcum / (double)G, prec[n] = tpcum / (double)(n + 1).  VOCap: the running maximum of
 * [0; prec; 0] from the end, mrec = [0; rec; 1], ap = the sum of (mrec(i) - mrec(i-1)) * mpre(i) over the i where mrec changes,
 * from 0.0 in ascending i, each product and addition rounded on its own.  Outputs apk[nparts] and, unless NULL, prec and rec
 * = double[nparts][capacity] (ncand for the host form), the first n of each row written.  An empty list gives apk = 0.  The
 * device form writes *d_status = the record count, or -1 for a word 0 that is negative or above capacity, and then nothing else;
 * a record whose frame is out of range is a false positive there (the host form refuses it).  The order costs one comparison
 * per pair of records. */
int pbd_eval_apk(pbd_handle *h, int nframes, const int32_t *gt_offset, const double *gt_points, const double *gt_scale, double thresh,
                 const int32_t *cand, int ncand, int frame_offset, double *apk, double *prec, double *rec);
int pbd_eval_apk_device(pbd_handle *h, int nframes, const int32_t *gt_offset, const double *gt_points, const double *gt_scale,
                        double thresh, const int32_t *d_payload, int capacity, int frame_offset, double *d_apk, double *d_prec,
                        double *d_rec, int32_t *d_status);

/* Candidate mask (new surface; opt-in): Candidate::mask(im, candidates, mask) (include/Candidate.hpp:306-331) and the ROS node's
 * masked colour frame `rgb & (mask != 0)` (ros/Messages.cpp:157-174, topic <name>/mask), for records of this handle spanning
 * several frames.  A record's frame index is `frame` - frame_offset (as pbd_boxes3d); frame f is im_rows[f] x im_cols[f]
 * (1..65536 each).  Records must be grouped by ascending frame (what pbd_suppress* produces); n is a record's 0-based position
 * among its frame's records in list order.
 *   box      boundingBox(): the hull of the record's nparts part rectangles under cv::Rect operator| (an empty accumulator takes
 *            the next rectangle as it is; an empty rectangle adds nothing), & Rect(0, 0, im_cols, im_rows); an empty
 *            intersection paints nothing
 *   label    min(1 + n_first, 255), n_first the smallest n whose box covers the pixel (setTo(n+1, mask == 0) with
 *            saturate_cast<uchar>); 0 where no box covers it.  Records from n = 254 on all paint 255 where nothing earlier did:
 *            lists of any length (an unsuppressed list) are valid
 *   masked   for 8-bit frames of `channels` 1, 3 or 4 interleaved bytes (the reference's case is 3, BGR): every byte of a pixel
 *            & (label != 0 ? 0xFF : 0).  masked[f] == colour[f] with the same pitch (in place) is allowed; otherwise the two
 *            must not overlap
 * Outputs, per frame: labels[f], uint8 rows x cols at label_pitch[f] bytes, and masked[f] at masked_pitch[f]; `labels` or
 * `masked` NULL omits that output (colour / colour_pitch / channels are then not read).  Pitches are at least the row's bytes.
 * pbd_candidate_mask: host records, frames and outputs, synchronous.  PBD_ERR_INVALID naming the index: a record whose frame
 * index is out of range or below its predecessor's, or whose nparts is outside 1..max parts; a frame whose size is outside
 * 1..65536 or whose pitch is below its row bytes; channels other than 1, 3 or 4 (with masked given).
 * pbd_candidate_mask_device: the records of the payload d_payload (word 0 = count, capacity records: what
 * pbd_detect_batch_device_out / pbd_suppress_device leave), device frames read in place (a frame may be a region of a larger
 * device image), device outputs.  Frame sizes and pitches are host arguments, validated as above.  Asynchronous on
 * pbd_stream(), no host synchronisation; the handle's workspace grows with capacity and nframes.  d_status int32[1]: the
 * record count, or -1 for a bad list -- a word 0 that is negative (a suppression overflow) or > capacity (a truncated list), a
 * frame index out of range or not grouped ascending, or (project decision) an nparts outside 1..max parts -- and then no
 * output is written.  The kernels' work is bounded by the tiles times the records scanned until a tile is covered, never by
 * pixels x records.
 * PBD_ERR_STATE while a batch is in flight; the resident detect result is not touched. */
int pbd_candidate_mask(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *cand, int ncand,
                       int frame_offset, uint8_t *const *labels, const size_t *label_pitch, int channels, const uint8_t *const *colour,
                       const size_t *colour_pitch, uint8_t *const *masked, const size_t *masked_pitch);
int pbd_candidate_mask_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *d_payload,
                              int capacity, int frame_offset, uint8_t *const *d_labels, const size_t *label_pitch, int channels,
                              const uint8_t *const *d_colour, const size_t *colour_pitch, uint8_t *const *d_masked,
                              const size_t *masked_pitch, int32_t *d_status);

/* Part-centre poses (new surface; opt-in): PartsBasedDetectorNode::messagePoses (ros/Messages.cpp:187-234, topic
 * <name>/object_poses) per record, on what pbd_boxes3d_camera* writes: centres float[3*max_parts*n] (record i, part j at
 * 3*(i*max_parts + j)), ncentres int32[n], dense int32[n].  PCL is not pinned; this is the library's contract, modelled on the
 * plain single-pass pcl::computeMeanAndCovarianceMatrix.  Every operation below is rounded on its own, in the order written.
 *   points   dense != 0: the first ncentres points, all of them (PCL's dense branch: an Inf point makes the result NaN);
 *            otherwise only those whose x, y and z are finite.  count = the points used
 *   moments  nine fp32 sums from 0 in point order: {xx, xy, xz, yy, yz, zz, x, y, z} (x*x etc. in fp32), each / (float)count.
 *            position = (m_x, m_y, m_z); C_ab = m_ab - m_a * m_b in fp32 (C symmetric); then C_ab /= (float)count again: the
 *            node's second division (covMat /= point_count, :212), kept on purpose
 *   frame    C widened to double; 8 cyclic Jacobi sweeps exactly as the plane fit of pbd_remove_planes (above); eigenvalues the
 *            diagonal in ascending order (pcl::eigen33's order), ties in index order.  Project decision (PCL's eigenvector signs
 *            are not pinned): columns 0 and 1 are the eigenvectors of the two smallest, each negated when its largest-magnitude
 *            component (the first on ties) is negative; column 2 = column 0 x column 1 in double, so the frame is a rotation
 *   quat     Eigen's Quaternion(const Matrix3 &) in double on the frame m: trace (m00 + m11) + m22 > 0: t = sqrt(trace + 1),
 *            w = 0.5 t, t = 0.5 / t, x = (m21 - m12) t, y = (m02 - m20) t, z = (m10 - m01) t; otherwise i = the largest diagonal
 *            (0, then 1 if m11 > m00, then 2 if m22 > m_ii), j = (i+1)%3, k = (j+1)%3, t = sqrt(((m_ii - m_jj) - m_kk) + 1),
 *            q_i = 0.5 t, t = 0.5 / t, w = (m_kj - m_jk) t, q_j = (m_ji + m_ij) t, q_k = (m_ki + m_ik) t.  Then each / sqrt(((x*x
 *            + y*y) + z*z) + w*w) (normalize()), rounded to float
 * Outputs per record: count int32 (0: "Centroid not found", the node's `continue`), position float[3], orientation float[4]
 * {x, y, z, w} (Eigen's coefficient order and geometry_msgs/Quaternion's), eigenvalues float[3] ascending.  count 0: position,
 * orientation and eigenvalues are NaN.  Project decision: an entry of C that is not finite makes the orientation and the
 * eigenvalues NaN (the position stays the means).
 * pbd_part_poses: host arrays of n records, synchronous; an ncentres outside 0..max parts is PBD_ERR_INVALID naming the record.
 * pbd_part_poses_device: device arrays read in place, min(max(word 0, 0), capacity) records of d_payload (the payload the
 * centres were computed from); an ncentres outside 0..max parts reads no point (count 0).  Asynchronous on pbd_stream().
 * PBD_ERR_STATE while a batch is in flight; the resident detect result is not touched. */
int pbd_part_poses(pbd_handle *h, int n, const float *centres, const int32_t *ncentres, const int32_t *dense, int32_t *count,
                   float *position, float *orientation, float *eigenvalues);
int pbd_part_poses_device(pbd_handle *h, const int32_t *d_payload, int capacity, const float *d_centres, const int32_t *d_ncentres,
                          const int32_t *d_dense, int32_t *d_count, float *d_position, float *d_orientation, float *d_eigenvalues);

/* Training examples (new surface; opt-in): the feature vector `ex` that the reference's Matlab training code builds from a
 * detection (matlab/detection/detect.m backtrack with write, qp_write), so that w . ex reproduces the detection's score.
 * The model vector: ONE parameter order per handle, values of T (the handle's real type), from the pbd_model the handle was
 * created with:
 *   w = [ biasw (nbias) | defw (ndefs x 4) | filters ]
 *   bias b at b, deformation d at nbias + 4 d, filter f at nbias + 4 ndefs + filter_offset[f], each k x (k * flen) row-major as
 *   pbd_model holds it; gaps between filters (a filter_offset table that does not pack them) are 0.
 * The `.i` offsets of a Matlab model are not used (as in the .mat reader).  pbd_model_vector_len: the number of values;
 * pbd_model_vector writes them to w (a host buffer of that many T).
 * An example: the walk of a record (frame, level, component, root_x, root_y) through the resident back-pointer maps, with the
 * pointer composition of pbd_detect*'s own walk (root mixture = the root's rooti, child position = Ix / Iy composed as the
 * reference does, include/DistanceTransform.hpp:233-244).  Per part, in part order 0..nparts-1, the blocks:
 *   bias    1 value = 1 at the bias the dynamic program added: the root's biasid of mixture 0 (src/DynamicProgram.cpp:163-170);
 *           a child of mixture mm under parent mixture m: biasid[c][p][mm] + m
 *   def     children only: 4 values {-dx*dx, -dx, -dy*dy, -dy}, dx = parent x + anchor x - x, dy likewise (the displacement
 *           the distance transform charged), so defw . def is the deformation term the transform added
 *   filter  the k x k x flen window of the feature map the convolution read for the part's response: cells x - k/2 .. and
 *           y - k/2 .. (OpenCV's centred anchor), row-major, channel fastest; a cell outside the map holds the convolution's
 *           border values: 0 on channels 0..flen-2, 1 on channel flen-1 (src/SpatialConvolutionEngine.cpp:146-156)
 * A block's offset is its place in w; two blocks may share an offset (a filter id used twice), as the score counted it twice.
 * Output per example i (record i of the caller's list), fixed strides reported by pbd_example_stride:
 *   hdr     int32[hdr_words] = {i, component, nblocks, nvalues, (offset, length) x nblocks, 0 ...}
 *   values  T[values]: the blocks' values concatenated in block order; values past nvalues are not written
 * w . values equals the record's score up to rounding (DESIGN.md section 6h states the bound) whenever the composed pointers
 * are the transform's true arg-max; where the reference's composition moved a part (a known quirk, reproduced on purpose)
 * the example is that of the placement the record reports and w . values is at most the score.  In PBD_WALK_ARGMAX
 * (pbd_set_walk) the walk is the arg-max and the identity holds for every record.
 * pbd_examples: host records (any subset of the last completed detect call's, in any order, with or without pbd_set_nms,
 * pbd_detect_frames' included); a record's frame is its `frame` field - frame_offset.  PBD_ERR_INVALID, naming the record,
 * when its frame, level, component or root position is outside the resident result (a level-sharded handle holds only its
 * own levels); PBD_ERR_STATE without a resident detect result (none yet, after pbd_conv_set_filters or pbd_dp_min, or a bank
 * whose filter sizes differ from the model's) or while a batch is in flight.  Synchronous.
 * pbd_examples_device: the records of the payload d_payload (word 0 = count, as pbd_detect_batch_device_out leaves it):
 * min(max(word 0, 0), capacity) examples, so a -1 payload writes nothing; a record outside the resident result gets the
 * header {i, component, -1, 0, 0 ...} and no values.  d_hdr = int32[capacity * hdr_words], d_values = T[capacity * values] on
 * the device.  Asynchronous on pbd_stream().  Neither call changes the resident result. */
/* Latent positives (new surface; opt-in): detect(im, model, 0, bbox, overlap) of the reference's Matlab training code
 * (matlab/learning/train.m poslatent; testoverlap, bbox.m).  Frames as pbd_detect_frames takes them (host pointers, mixed sizes,
 * the four depths, nframes <= max_batch).  boxes = int32[nframes][nparts][4]: frame f's ground-truth box {x1, y1, x2, y2}
 * (inclusive, as in Matlab) of every part index; mixtures = int32[nframes][nparts] fixed mixture of every part (-1 free), or NULL.
 * Part p (of every component) at (x, y) of level l with mixture m keeps its response only when m is allowed and its record
 * rectangle (src/DynamicProgram.cpp:238-241: xy1 = ((x, y) - (1, 1)) * scale, xy2 = xy1 + size(m) * scale - (1, 1), cvRound;
 * the rectangle of min / max corners) passes inter / (area + barea - inter) > overlap, computed in double with inclusive (+1)
 * areas; otherwise the response is replaced by -1e10 in T (Matlab's -INF, finite: -inf would put NaN into the transform's
 * intersections).  PBD_CONV_MFMA_F16_ANY, whose responses are fp16, replaces it by -65504, the most negative finite fp16 value,
 * and reports found[f] = 1 iff the score > -32752: right as long as the unmasked terms of a root sum to less than 32752.  The mask belongs to the (component, part, mixture): the call runs the model with one filter per
 * (component, part, mixture) (filter ids shared by several parts are copied), the sequential schedule of shared ids does not
 * apply, and the detect path of the handle is not touched.  Output per frame f: cand + f * pbd_candidate_stride() = the single
 * highest-scoring root over all levels, components and positions (ties: the first in (level, component, y, x) order), as a
 * normal record (`frame` = f, part boxes of the walk); found[f] = 1 iff its score > -5e9 (no masked term used).
 * The level images stay in the twin: pbd_get_pyramid_image gives PBD_ERR_STATE after it.
 * The call leaves a resident result: pbd_examples* then give the positives' feature vectors (offsets in this handle's model
 * vector) and pbd_get_stage reads the stages of that run, addressed (frame, level) as after a mixed call: PBD_STAGE_RESPONSES is
 * the MASKED responses, one plane per (component, part, mixture) in global mixture order; PBD_STAGE_ROOTV / _ROOTI are the
 * dynamic program's on them and PBD_STAGE_FEATURES the frames' features.  pbd_argmin_device_out / pbd_dp_argmin see no result
 * until the next detect call.  pbd_set_nms does not apply.
 * PBD_ERR_UNSUPPORTED: components with different part counts, level sharding (world > 1), PBD_CONV_MFMA_F16 (mode 3; mode 6,
 * PBD_CONV_MFMA_F16_ANY, is taken as said above).
 * PBD_ERR_INVALID: a NaN overlap, and the frame refusals of pbd_detect_frames.  PBD_ERR_STATE while a batch is in flight. */
int pbd_detect_latent(pbd_handle *h, int nframes, const struct pbd_frame *frames, int channels, int depth_code, const int32_t *boxes,
                      const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found);
int pbd_model_vector_len(const pbd_handle *h);
int pbd_model_vector(pbd_handle *h, void *w);
/* In-place model update (new surface; opt-in): model = vec2model(qp_w, model) of the reference's Matlab training code
 * (matlab/learning/train.m after every qp_opt; matlab/detection/detect.m:148-151, 316-325) without a new handle.  DESIGN.md
 * section 6j.  After a successful call the handle cannot be told apart from one that pbd_create builds, with the same config,
 * from the same pbd_model with its parameters replaced by w (Model.from_vector(w)): pbd_model_vector, the records of
 * pbd_detect*, pbd_get_stage, pbd_detect_latent and pbd_examples* are equal bit for bit, in every convolution mode and real type.
 * Topology, anchors, filter sizes and offsets, sbin, interval, thresh, plans, buffers, pbd_set_nms, pbd_set_level_shard and the
 * stream are not touched.  Rounding: that of pbd_create -- bias and deformation values to float32 (pbd_model holds them so),
 * filters to T; an F64 source into an F32 handle is rounded once per value.
 * pbd_set_model_vector: w = pbd_model_vector_len values of T on the host.
 * pbd_set_model_vector_device: d_w = that many float (real_code PBD_REAL_F32) or double (PBD_REAL_F64) values on the handle's
 *   device; the caller orders whatever wrote d_w before pbd_stream().
 * pbd_qp_apply: w_k / wreg_k + w0_k formed in double on the device (pbd_qp_weights' expression), then rounded as above;
 *   pbd_stream(h) waits for the QP's stream; nothing passes through the host.  Its message is pbd_qp_last_error(q).
 * The work runs on pbd_stream(): a check kernel, then kernels that rebuild every weight-dependent table of the handle (the
 * banks of each size class, the matrix-core fragments, the channel-31 border table, bias and deformation tables) and of its
 * latent twin, if pbd_detect_latent has created one, from the one device vector.  The call returns after reading back one
 * small status block (the refusal flag and the nbias + 4 ndefs float values the host keeps); in the device forms nothing of
 * the size of the filter bank crosses to the host (pbd_model_vector after an update fetches the vector when asked).
 * The resident detect result is dropped as after pbd_conv_set_filters: pbd_examples*, pbd_argmin_device_out and pbd_dp_argmin
 * give PBD_ERR_STATE until the next detect call.
 * Refusals, each leaving the handle unchanged: PBD_ERR_STATE while a batch is in flight, or after a pbd_conv_set_filters whose
 * bank no longer matches the model's filters; PBD_ERR_INVALID for a deformation (of a non-root part) whose quadratic term,
 * element 0 or 2, is zero once rounded to float32 (pbd_create's refusal, made on the device before anything is written), for
 * a pbd_qp whose layout fingerprint differs from the handle's or that lives on another device, for NULL pointers and for a
 * real_code that is neither PBD_REAL_F32 nor PBD_REAL_F64.
 * A HIP failure after the kernels were queued (PBD_ERR_HIP from an update) leaves tables that may be half new: the handle then
 * refuses every later update and detect call with PBD_ERR_STATE and must be destroyed.
 * pbd_set_thresh: the model's thresh (train.m: model.thresh = the 5th percentile of qp_scorepos) for every later detect call;
 * the resident result stays.  PBD_ERR_STATE while a batch is in flight. */
int pbd_set_model_vector(pbd_handle *h, const void *w);
int pbd_set_model_vector_device(pbd_handle *h, const void *d_w, int real_code);
int pbd_set_thresh(pbd_handle *h, float thresh);
int pbd_example_stride(const pbd_handle *h, int *hdr_words, int *values);
int pbd_examples(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, int32_t *hdr, void *values);
int pbd_examples_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_hdr, void *d_values);
/* Part scores (new surface; opt-in): what the dynamic program added up for a record, per part, and the placement (cell and
 * mixture of every part) it was added up at.  The reference's Candidate declares "bounding box and detection confidence for each
 * part" (include/Candidate.hpp:54-72) and its walk fills only the root's; these calls give the rest.  DESIGN.md section 6s; the
 * rule in numpy: partsbaseddetector_amd/partscores.py.
 * A record (frame, component c, level l) and a placement (x_p, y_p, m_p), p = 0 .. nparts-1, of the resident result.  T is the
 * handle's real type, gm(p) part p's global mixture index for m_p, f its filter id, d its deformation id:
 *   appearance[p] = the resident response resp_l[f][y_p][x_p] of the call, whatever convolution mode produced it (fp16 resident
 *                   responses, modes 3 and 6, widened to float)
 *   bias[p]       = the root: biasw[biasid of the root's mixture 0] (src/DynamicProgram.cpp:163-170); a child:
 *                   biasw[biasid[gm(p)] + m_parent]; float converted to T
 *   total[p]      starts as appearance[p]; then for q = nparts-1 down to 1, in that order (the reference's descending child order):
 *                   dx = x_parent + anchor_x[d] - x_q, dy likewise;
 *                   r = Q(-w0, -w1, dx, total[q]), message[q] = Q(-w2, -w3, dy, r), where Q(a, b, d, y) = (T)(a * (double)(d * d)
 *                   + b * (double)d + (double)y): the int square, double arithmetic left to right, ONE rounding to T per pass, as
 *                   the transform's row and column passes round (include/DistanceTransform.hpp:102-104);
 *                   total[parent] = total[parent] + (message[q] + bias[q]), both adds in T
 *   message[0]    = total[0] + bias[0] in T
 * Output per (record, part): T[4] = {appearance, message, bias, total}.  message[q] - total[q] is the deformation part q paid, to
 * one rounding.
 * Guarantees:
 *  1. PBD_WALK_ARGMAX, a model in which no part that has children shares a filter id with another part of its component (every
 *     model pbd_create is given by build_model / trainmodel()): for every record (float)message[0] has the bits of the record's
 *     score, and total[p] is the value the dynamic program accumulated for part p at its cell.
 *  2. PBD_WALK_REFERENCE: the values are those of the placement the record reports (the composed pointers may move a part off
 *     the arg-max), and (float)message[0] is that placement's own score: at most the record's, below it where a part was moved.
 *  3. Inner parts that share a filter id (the reference keys its accumulators by filter id, src/DynamicProgram.cpp:115-119,
 *     154-156, so such a plane holds both parts' messages): the four values are still exactly the rule's; the equalities of (1)
 *     are not promised.
 * pbd_part_scores: host records, any subset in any order of the last completed detect call's (with or without pbd_set_nms,
 * pbd_set_root_nms, pbd_set_depth_prune, pbd_set_top_k; pbd_detect_frames' and pbd_detect_latent's included: after the latter the
 * responses are the masked ones of its one-filter-per-mixture run).  The placement is the walk's in the handle's walk mode
 * (pbd_set_walk), as pbd_examples walks.  status = int32[ncand]: the record's parts; place = int32[ncand][max_parts][3] {x, y, m}
 * (may be NULL); scores = T[ncand][max_parts][4].  Entries past a record's parts are not written.  Refusals are pbd_examples':
 * PBD_ERR_INVALID naming the record, PBD_ERR_STATE without a resident result or while a batch is in flight.  Synchronous.
 * pbd_part_scores_device: min(max(word 0, 0), capacity) records of the payload d_payload, so a -1 payload writes nothing; a
 * record outside the resident result gets status -1 and nothing else.  Device arrays of `capacity` records (d_place may be NULL).
 * Asynchronous on pbd_stream().
 * pbd_score_placements / _device: the same values at placements the caller gives (place[i][0] is the root): frame, level and
 * component are the record's, its root cell is ignored.  A placement with a cell outside the level's map or a mixture outside the
 * part's range gets status -1 and no values; the other records of the call are not affected.
 * No call changes the resident result. */
int pbd_part_scores(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, int32_t *status, int32_t *place, void *scores);
int pbd_part_scores_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_status, int32_t *d_place,
                           void *d_scores);
int pbd_score_placements(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, const int32_t *place, int32_t *status,
                         void *scores);
int pbd_score_placements_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, const int32_t *d_place,
                                int32_t *d_status, void *d_scores);
/* Max-marginals of every part and the poses they decode to (new surface; opt-in).  DESIGN.md section 6t; the rule in numpy:
 * partsbaseddetector_amd/marginals.py.  The detector answers "the best configuration rooted at this cell"; the max-marginal
 * mm_p[m][y][x] answers it for every part: the score of the best configuration with part p of type m at (x, y).
 * Per (frame, level, component) on the level's H x W maps; T the handle's real type, q = parent(p), K_p the types of p, every +
 * one addition rounded to T, a bias entering as (T)biasw[..]:
 *   S_p[m]    the plane part p, type m, had accumulated when the upward pass consumed it (a leaf: its filter's response)
 *   D_p[m]    = dt(S_p[m]; -w0, -w1, -w2, -w3; ox, oy), the upward transform (rows pass, then columns pass)
 *   M_p[mq]   = reduceMax over m of (D_p[m] + bias(p, m)[mq]): strict >, the first of equals wins, K_p == 1 copies
 *   root      down_0[m] = (T)bias of the root's type 0 for every root type m; mm_0[m] = S_0[m] + down_0[m]
 *   context   C_p[mq] = resp(filter(q, mq)); for every child c of q in DESCENDING index order, c != p: C_p[mq] += M_c[mq]; last
 *             C_p[mq] += down_q[mq]
 *   mirrored  R_p[m][mq] = dt(C_p[mq]; -w0, +w1, -w2, +w3; -ox, -oy) with the weights and anchor of (p, m): the upward quadratic
 *             seen from the child (the negated linear coefficients: an upward -0.0 becomes +0.0), the transform otherwise the
 *             upward one, the NaN read-out rule of pbd_dp_min included ("Non-finite scores", item 3: +-Inf and NaN responses are
 *             accepted; a context plane may hold NaN the upward pass never saw, from -Inf + +Inf; NaN in mm and down stand at the
 *             places of the rule run with that read-out, sign and payload unspecified; the pointer planes are the rule's.  With
 *             K_q > 1 a NaN never wins the reduction, so down is -inf and Jk 0 where every R + bias is NaN or -inf)
 *   down      down_p[m] = reduceMax over mq of (R_p[m][mq] + bias(p, m)[mq]), the same first-wins rule and K_q == 1 copy;
 *             Jk_p[m] the winning mq; (Jx_p[m], Jy_p[m]) the parent's cell, composed in arg-max order from the winner's pointer
 *             planes: the columns pass's pointer first, then the rows pass's at that row
 *   mm        mm_p[m] = S_p[m] + down_p[m]
 * so reduceMax over m of mm_0[m] has the bits of the root scores (and its index is their type), and where every sum is exact in
 * T, mm_p[m][y][x] is exactly the maximum over the configurations with p of type m at (x, y).
 * pbd_max_marginals(h, frame): the planes of one frame of the resident dynamic-program result (after pbd_detect*, equal-size
 *   frames, or pbd_dp_min: frame 0), kept on the device until the next detect call, pbd_dp_min, model update or
 *   pbd_max_marginals.  Asynchronous on pbd_stream().  The resident detection result is not changed.
 *   The planes belong to the result they were computed from:
 *   every call that replaces, cuts or drops the resident result drops the marginals with it
 *   (pbd_features_pyramid, pbd_conv_pdf, pbd_conv_set_filters, pbd_detect_latent and pbd_warp_positives as well).  Device memory held:
 *   (2 sizeof(T) + 5) NJ + sizeof(T) NS bytes per cell of the frame, plus scratch of sizeof(T) JGmax + 2 P max(JGmax, NJ) bytes per
 *   cell (NJ: the (part, type) pairs of the model, NS its pointer slots, JGmax the transforms of its largest depth group, P the
 *   bytes of a position: 1 while no map side exceeds 256, else 2).
 *   PBD_ERR_STATE: no resident dynamic-program result (none yet, after a model update or pbd_conv_set_filters), a latent result
 *   (pbd_detect_latent), a batch in flight.  PBD_ERR_INVALID: frame outside the result.  PBD_ERR_UNSUPPORTED: a model on the
 *   sequential schedule (a filter id shared inside a component), fp16-resident responses (modes 3 and 6), a mixed-size result
 *   (pbd_detect_frames), a level-sharded handle (world > 1), a padded result (pbd_set_padding; pbd_get_marginals,
 *   pbd_marginals_device and pbd_marginal_poses* refuse it likewise).
 * pbd_get_marginals(h, level, what, dst, dst_bytes): one level's block, synchronous.  PBD_MM_VALUES / PBD_MM_DOWN: T[NJ][H][W];
 *   PBD_MM_PARENT_X / _Y / _K: int32[NJ][H][W], -1 in every plane of a root.  PBD_ERR_STATE without resident marginals.
 * pbd_marginals_device(h, level, &d): the device pointer of the level's mm block T[NJ][H][W] (for pbd_grid_nms_device /
 *   pbd_top_k_cells_device), valid as long as the marginals are.
 * pbd_marginal_poses(h, n, seeds, scales, frame_offset, cand, place, status): seeds = int32[n][6] {level, component, part, type
 *   or -1 (the first type with the largest mm at the cell; reduceMax's rule, so type 0 where no mm is above -inf: every one
 *   NaN or -inf), x, y}.  The pose of a seed: climb from the seed through Jk / Jx / Jy to
 *   the root, which fixes every part on that path; every other part, in index order, takes the arg-max placement of the upward
 *   pointers from its parent's (whatever pbd_set_walk says: the marginal was taken there).  cand = int32[n][stride] records:
 *   frame (that of pbd_max_marginals) + frame_offset, component, level, the decoded root's x, y, (float)mm of the seed (of the
 *   type decoded for a type of -1: a NaN or -inf where no type won; a NaN's sign and payload are unspecified), parts, the
 *   root's type in word 7, then the part boxes at the level's scale; scales = float[levels] as for pbd_dp_argmin, or NULL for the
 *   plan's own (after pbd_detect*; NULL after pbd_dp_min is PBD_ERR_INVALID).  place = int32[n][max_parts][3] {x, y, type} or
 *   NULL.  status = int32[n]: the parts of the pose, or -1 for a bad seed (a cell outside the map, a part, type, component or
 *   level out of range), whose record and placement are not written.  Synchronous; pbd_marginal_poses_device takes device
 *   arrays and is asynchronous on pbd_stream().  PBD_ERR_STATE without resident marginals. */
enum { PBD_MM_VALUES = 0, PBD_MM_DOWN = 1, PBD_MM_PARENT_X = 2, PBD_MM_PARENT_Y = 3, PBD_MM_PARENT_K = 4 };
int pbd_max_marginals(pbd_handle *h, int frame);
int pbd_get_marginals(pbd_handle *h, int level, int what, void *dst, size_t dst_bytes);
int pbd_marginals_device(pbd_handle *h, int level, void **d_values);
int pbd_marginal_poses(pbd_handle *h, int n, const int32_t *seeds, const float *scales, int frame_offset, int32_t *cand,
                       int32_t *place, int32_t *status);
int pbd_marginal_poses_device(pbd_handle *h, int n, const int32_t *d_seeds, const float *scales, int frame_offset, int32_t *d_cand,
                              int32_t *d_place, int32_t *d_status);
/* Warped positives (new surface; opt-in): poswarp of the reference's Matlab training code (matlab/learning/train.m:131-162 with
 * matlab/learning/warppos.m, subarray.m and qp_poswrite), the examples every training run starts from (trainmodel.m:19-40 trains
 * each part mixture as a one-part model on them).  DESIGN.md section 6k.  Each annotated box is padded by one cell, cropped with
 * edge replication, resized to (k + 2) * sbin pixels, and its HOG written as an example in pbd_examples' format.  Mirrored
 * and rotated copies are made by pbd_augment_frames* (below), not here (the train() loop over these calls
 * is partsbaseddetector_amd/train.py).
 * Frames as pbd_detect_frames takes them: host pointers (pbd_warp_positives) or device pointers (the _device form), mixed sizes,
 * one `channels` (1 or 3) and one depth_code (all four) per call; a _device frame may be a region of a larger device image, read
 * in place through its pitch, its pointer and stride_bytes multiples of the element size.  A frame only has to be 1 x 1 or
 * larger (no pyramid of it is planned) and nframes is not bound by max_batch.
 * boxes = int32[nboxes][5] = {frame, x1, y1, x2, y2}, always a host array; 0-based inclusive corners as the boxes of
 * pbd_detect_latent.  Several boxes may name one frame, in any order; a frame may have no box.
 * Window of box i, with k = filter_ksize[filter], s = sbin, width = x2 - x1 + 1, height = y2 - y1 + 1:
 *   padx = s * width / (k * s), pady = s * height / (k * s), left to right in double (warppos.m:21-22);
 *   in Matlab's 1-based coordinates X1 = round((x1 + 1) - padx), X2 = round((x2 + 1) + padx), Y1 and Y2 likewise, round = halves
 *   away from zero (Matlab's); the 0-based window is columns X1-1 .. X2-1, rows Y1-1 .. Y2-1, and its pixel (r, c) is the frame's
 *   pixel (clamp(Y1-1+r, 0, rows-1), clamp(X1-1+c, 0, cols-1)): subarray(im, Y1, Y2, X1, X2, 1).  rows and cols are the frame's
 *   own (a region of a larger image is clamped at the region, not at its parent).
 * Patch: the window resized to P x P, P = (k + 2) * s, by this library's cv::resize INTER_LINEAR restatement with the
 *   coefficient arithmetic of a resized pyramid level of the same depth (source size = the window's, destination size = P).  No
 *   crop is materialised: the taps index the window and the clamp maps them into the frame.
 * Features: HOGFeatures<T>::features(patch) at sbin; blocks = k + 2 exactly, so the result is k x k x flen, row-major, channel
 *   fastest: the layout of a filter in the model vector.
 * Project decisions: Matlab's imresize(..., 'bilinear') is not reproduced (toolbox code that antialiases when shrinking and
 *   works in double; nothing here can pin it), nor is the double-precision mex features.cc.  The example holds what this detector
 *   computes on that patch, so a filter trained on it meets the same features at detection time.  A one-channel frame is used as
 *   the handle's HOG uses one (Matlab's repmat to three equal channels gives the same gradients).
 * Skip rule: with skip_small != 0 a box with (double)width * height < ((double)k * s)^2 is skipped (train.m:135-143 with
 *   minsize = prod(model.maxsize * model.sbin)).
 * Example of a kept box i, pbd_examples' format and strides (pbd_example_stride):
 *   hdr = {i, 0, nblocks, nvalues, (offset, length) x nblocks, 0 ...}; with bias >= 0 the blocks are (bias, 1) holding 1, then
 *   (nbias + 4 ndefs + filter_offset[filter], k * k * flen) holding the features (qp_poswrite's order); with bias == -1 only the
 *   filter block.  Values past nvalues are not written.
 * A skipped box gets hdr = {i, 0, -1, 0, 0 ...} and no values: the invalid marker pbd_qp_add_device skips.
 * pbd_warp_positives: hdr int32[nboxes][hdr_words], values T[nboxes][values] and kept int32[nboxes] (1 / 0) on the host.
 *   Synchronous.
 * pbd_warp_positives_device: d_hdr / d_values as pbd_examples_device; d_payload = int32[1 + capacity * pbd_candidate_stride()],
 *   word 0 = nboxes, record i = {frame = id_offset + i, component 0, level 0, root_x 0, root_y 0, score 0, nparts 0, 0, zeros},
 *   so that pbd_qp_add_device(q, h, d_payload, capacity, d_hdr, d_values, 1, id_base, ...) writes the ids
 *   {1, id_base + id_offset + i, 0, 0, 0} (ex.id = [1 id 0 0 0]).  nboxes > capacity: PBD_ERR_CAPACITY before anything is
 *   enqueued.  Asynchronous on pbd_stream() (the call returns once its tap tables, 28 P bytes per kept box for 8-bit frames
 *   and 40 P for the other depths, are staged in pinned memory and the kernels are enqueued).
 * Refused before anything is enqueued, naming the offending index, the handle unchanged: PBD_ERR_INVALID for a filter outside
 *   0..nfilters-1, a bias outside -1..nbias-1, a box whose frame index is outside 0..nframes-1 or with x2 < x1 or y2 < y1 or a
 *   coordinate outside +-2^24 (the tap positions are floats), the frame refusals of pbd_detect_frames (a NULL or empty frame, a
 *   pitch below the row, channels other than 1 or 3, a misaligned device frame; PBD_ERR_UNSUPPORTED for another depth_code) and
 *   its NaN / Inf refusal for host 32F / 64F frames, NULL pointers with nboxes > 0, nboxes < 0; PBD_ERR_STATE while a batch is
 *   in flight or after a pbd_conv_set_filters whose bank no longer matches the model.  nboxes == 0 is PBD_OK (the device
 *   payload's word 0 is then 0).
 * The call works in the handle's pyramid and HOG workspaces, so the resident detect result is dropped as after
 * pbd_conv_set_filters: pbd_get_stage, pbd_examples*, pbd_argmin_device_out and pbd_dp_argmin give PBD_ERR_STATE until the next
 * detect call (a refused call and a call with nboxes == 0 leave it).  The detect path itself is untouched: a detect call gives
 * the same bytes before and after.  Nothing of the dropped result stays readable, its features and level images neither:
 * pbd_get_pyramid_image, pbd_part_scores*, pbd_score_placements* and pbd_max_marginals likewise give PBD_ERR_STATE. */
int pbd_warp_positives(pbd_handle *h, int nframes, const struct pbd_frame *frames, int channels, int depth_code, int nboxes,
                       const int32_t *boxes, int filter, int bias, int skip_small, int32_t *hdr, void *values, int32_t *kept);
int pbd_warp_positives_device(pbd_handle *h, int nframes, const struct pbd_frame *d_frames, int channels, int depth_code, int nboxes,
                              const int32_t *boxes, int filter, int bias, int skip_small, int id_offset, int32_t *d_payload,
                              int capacity, int32_t *d_hdr, void *d_values);
/* Augmented positives (new surface; opt-in): the rotated and mirrored copies the reference's training pipeline multiplies its
 * positives by (matlab/globals.m:18-23 imrotate/ and imflip/, matlab/learning/map_rotate_points.m, train.m:130,165; the step
 * itself, PARSE_data.m, is not in the reference).  DESIGN.md section 6r; the numpy yardstick is partsbaseddetector_amd/augment.py.
 * A copy of a frame (rows x cols x channels, any of the four depths) is rotate(mirror(frame)):
 *   mirror   column q becomes cols - 1 - q.
 *   rotate   degrees == 0: none, the copy has the frame's size.  Otherwise (map_rotate_points.m:20-35) (c, s) = (cos, sin) of
 *     degrees * pi / 180 in double, exactly {0, +-1} for multiples of 90; hA = ((rows - 1) / 2, (cols - 1) / 2); the corners
 *     (-hAr, hAc) and (hAr, hAc) as row vectors times [c s; -s c]; hB = ceil(max|.| / 2) * 2 per axis; the copy is
 *     (2 hBr + 1) x (2 hBc + 1).  Its pixel (R, Q) is the source's pixel (floor(r + 0.5), floor(q + 0.5)) with
 *     r = (R - hBr) c + (Q - hBc) s + hAr, q = -((R - hBr) s) + (Q - hBc) c + hAc (every product rounded, sums left to right),
 *     all bytes 0 outside the source: nearest neighbour, positive angles counter-clockwise.  imrotate's toolbox code is not
 *     reproduced (bilinear and cropped rotation are out of scope).
 * pbd_augment_plan: the copy's size and coef = {c, s}, the coefficients the kernel uses.  Pure host code.
 * pbd_augment_points: npoints points {x, y} (0-based, real) of the frame mapped into the copy: x -> cols - 1 - x when mirror,
 *   then the forward map of map_rotate_points.m:40.  xy_out may be xy.  Pure host code.  Both: PBD_ERR_INVALID for a size
 *   outside 1..32000 or non-finite degrees.
 * pbd_augment_frames*: njobs copies in ONE launch; job i = {frame, mirror, degrees} writes out[i].  Frames as
 *   pbd_warp_positives* takes them (host or device pointers, mixed sizes and pitches, device regions of larger images, channels 1
 *   or 3, the four depth codes); several jobs may name one frame, a frame may have no job.  Destination bytes beyond a row's
 *   used width are not written.  pbd_augment_frames: host frames and destinations, synchronous.  pbd_augment_frames_device:
 *   device frames and destinations (pointer and pitch multiples of the element size), asynchronous on pbd_stream().
 * Refused before anything is enqueued, naming the offending index: PBD_ERR_INVALID for a job whose frame index is out of range,
 *   non-finite degrees, a destination whose rows or cols differ from the plan's, whose pitch is below its row, that is NULL or
 *   (device) misaligned, or that overlaps one of the call's frames; the frame refusals of pbd_detect_frames; PBD_ERR_STATE while
 *   a batch is in flight.  njobs == 0 is PBD_OK.  The call has buffers of its own: the resident detect result and the detect
 *   path are not touched. */
struct pbd_augment { int32_t frame; int32_t mirror; double degrees; };
int pbd_augment_plan(int rows, int cols, double degrees, int *out_rows, int *out_cols, double coef[2]);
int pbd_augment_points(int rows, int cols, double degrees, int mirror, int npoints, const double *xy, double *xy_out);
int pbd_augment_frames(pbd_handle *h, int nframes, const struct pbd_frame *frames, int channels, int depth_code, int njobs,
                       const struct pbd_augment *jobs, const struct pbd_frame *out);
int pbd_augment_frames_device(pbd_handle *h, int nframes, const struct pbd_frame *d_frames, int channels, int depth_code, int njobs,
                              const struct pbd_augment *jobs, const struct pbd_frame *d_out);
/* pbd_detect_latent with device frame descriptors (pointer and pitch multiples of the element size; regions of larger device
 * images included), read in place.  boxes, mixtures, cand and found stay host arrays and the call is synchronous; every refusal
 * and the resident result afterwards are those of pbd_detect_latent (the NaN / Inf refusal reads host pixels and does not apply). */
int pbd_detect_latent_device(pbd_handle *h, int nframes, const struct pbd_frame *d_frames, int channels, int depth_code,
                             const int32_t *boxes, const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found);

/* ---- Training QP (new surface; opt-in): the dual coordinate-descent solver of the reference's Matlab training code
 * (matlab/learning/qp_write.m, qp_one.m with oct/qp_one_sparse.cc, qp_opt.m, qp_refresh.m with oct/lincomb.cc, qp_prune.m,
 * qp_w.m, model2vec.m) over a cache of examples that stays on the device.  DESIGN.md section 6i.
 * A pbd_qp owns its device memory and outlives the handle it was created from: pbd_qp_create copies the handle's model-vector
 * layout (length, the block of every bias, deformation and filter, the example strides), its device and a fingerprint of the
 * layout, nothing else.  Examples of any handle with the same fingerprint (float or double) may be added.
 * The problem, in the standard form of qp_write: min_v 1/2 |v|^2 + sum_groups max(0, max_{i in group} b_i - v . x'_i), with
 * v = (w - w0) .* wreg; the dual keeps a_i in [0, 1] with sum over a group <= 1 (C = 1 per group, as qp_one passes it).
 * Config: capacity (examples, >= 1); C and wpos (0 selects the defaults 0.002 and 2; Cpos = C * wpos, Cneg = C; NaN, infinite
 * or negative values are PBD_ERR_INVALID); stream (NULL: the QP creates its own); wreg, w0 (double[len]) and noneg
 * (int32[nnoneg] indices into w): NULL selects model2vec's defaults in this library's vector order: wreg = 0.01 on every
 * component's root bias (biasid of part 0, mixture 0), 1 elsewhere; w0 = 0.01 and non-negativity on elements 0 and 2 of every
 * deformation block (-dx^2, -dy^2).
 * A cache entry i: ids[i] (5 int32), x'_i (float32, block-sparse: {nblocks, nvalues, (offset, length, first value) x nblocks}),
 * b_i and d_i (double), a_i (double), sv_i.  Entries 0..nfix-1 are fixed support vectors (pbd_qp_fix).
 * pbd_qp_add / pbd_qp_add_device (qp_write, for each example in order while the cache has room; the number written goes to
 * *taken / *d_taken, examples past capacity are dropped silently as qp_write drops them, nothing is written past capacity):
 *   label = ids[0] > 0; Cl = Cpos if label else Cneg; blocks with one offset are merged into the first of them by summing
 *   their values in block order in double (a filter id used twice; w . x is unchanged); x = the merged values, negated when
 *   !label; x'_j = float32((Cl * x_j) / wreg_j) (double, rounded once); b = Cl * (1 - R(w0 . x)); d = R(x' . x'); a = 0,
 *   sv = 1 (a new slot starts at a = 0: train.m reuses slots with their stale a after qp.n = 0, which is not reproduced).
 *   An example is skipped and not counted when its header is marked invalid (nblocks -1, pbd_examples_device) or any block is
 *   not exactly a bias, deformation or filter block of the layout (pbd_qp_add refuses such a header with PBD_ERR_INVALID).
 *   pbd_qp_add: host hdr / values in pbd_examples' format and strides from handle h (values of h's T), ids int32[n][5].
 *   pbd_qp_add_device: the min(max(word 0, 0), capacity) examples of a pbd_examples_device call on h's payload; example i's id
 *   is {label, id_base + record frame, level, root x, root y} (detect.m's ex.id); the QP's stream waits for h's stream, the call
 *   is otherwise ordered on the QP's stream; d_taken: int32 on the device or NULL.  The call returns once the entries are
 *   written (the QP keeps the ids and block tables of its entries on the host, 20 + 4 * hdr_words bytes per entry).
 * R(.) is the reduction of every sum that decides a branch or a result: lane-strided partial sums, PBD_QP_LANES lanes, value j
 * of the example (in stored block order) going to lane j mod PBD_QP_LANES, each lane adding its products in ascending j from
 * +0.0; then per group of 64 consecutive lanes the halving tree s[l] = s[l] + s[l + h], h = 32, 16, ..., 1; then the halving
 * tree over the 16 group sums (h = 8, 4, 2, 1).  A product is a multiply then an add, never fused.  In x . x2 a value of x
 * whose coordinate x2 does not carry contributes +0.0.  w . w uses the same reduction over the dense w.
 * Grouping: entries with equal 5-word ids form a group.  Groups are numbered in ascending order of their first member.
 * pbd_qp_one: one pass of qp_one_sparse over the pass set S = {i < n : sv_i} (PBD_ERR_STATE when empty) in the order
 *   order[0..nsv) (a permutation of 0..nsv-1, indices into S ascending); order NULL: the stable argsort of
 *   splitmix64(seed, nsv) as partsbaseddetector_amd/synth.py defines it.  At the start of the pass, per group of S: idC = the
 *   sum of a over its members in ascending index, idI = its highest index with a > 0 (none: -1).  Each step is the mex loop's
 *   (oct/qp_one_sparse.cc:171-253) with G = R(w . x) - b, the paired update's G2 and x . x2 by R, w += dA x then w += (-dA) x2,
 *   then w[k] = w[k] < 0 ? 0 : w[k] on every non-negative k.  loss = the sum of the groups' err in group order.  Then refresh,
 *   sv = 1 on the fixed entries, lb = l - R(w . w) * 0.5, ub = R(w . w) * 0.5 + loss.
 * Refresh (qp_refresh): P = {i : a_i > 0} sorted by ascending a (ties: index); l = the sequential sum of b_i * a_i over P;
 *   w_k = the sequential sum over P of a_i * x'_ik over the entries carrying coordinate k (0 elsewhere; lincomb's order); the
 *   non-negativity clamps; lb = l - R(w . w) * 0.5.  lb below the previous lb - 1e-5 (the reference's assert) sets lb_dropped.
 * pbd_qp_opt: qp_opt: refresh, ub = R(w . w) * 0.5 + computeloss (over the whole cache: per group max(0, max of b - R(w . x)),
 *   summed in group order), sv = 1 on all; pass t = 0, 1, ... < iter is pbd_qp_one with seed + t, then with lb > 0 and
 *   1 - lb / min(pass ub, ub) < tol the true bound ub = min(ub, R(w . w) * 0.5 + computeloss); stop when 1 - lb / ub < tol,
 *   else sv = 1 on all.  state.ub = ub, state.passes, state.converged.  NaN tol: PBD_ERR_INVALID.
 * pbd_qp_fix: the fixed set becomes 0..n-1 and their sv = 1 (train.m: qp.svfix = 1:qp.n; qp.sv(qp.svfix) = 1).
 * pbd_qp_prune: qp_prune: when every entry is a support vector, sv = (a > 0) or fixed; the entries with sv are moved to the
 *   front in order (the fixed ones stay 0..nfix-1), sv = 1 on them, then refresh.  *n = the new count.  PBD_ERR_STATE when none.
 *   The move goes through a scratch buffer of at most 256 entries and 256 MB, freed before the call returns.
 * pbd_qp_weights: qp_w: w_k / wreg_k + w0_k in double (len values) for Model.from_vector / a new handle.
 * pbd_qp_scores: qp_scorepos: per positive entry (ids[0] > 0, ascending index) R((w + w0 .* wreg) . x') / Cpos; s holds
 *   capacity doubles, *n the count.
 * pbd_qp_state: the counters and bounds (struct pbd_qp_info); a (double[n]), sv (uint8[n]) and w (double[len]) when not NULL.
 * pbd_qp_entries: entries first..first+count-1: hdr int32[count][hdr_words], values float[count][values] (past nvalues 0),
 *   b, d double[count], ids int32[count][5]; any pointer may be NULL.
 * pbd_qp_clear: train.m:75's qp.n = 0 for the next iteration: n = 0, nfix = 0, l = loss = 0, lb = ub = NaN, passes, converged
 *   and lb_dropped 0, a = 0 and sv = 0 on every slot, the host tables emptied -- the state after pbd_qp_create.  w is left as it
 *   is; the next refresh rebuilds it.  New slots start at a = 0, as always (the stale qp.a of train.m is not reproduced).
 * pbd_qp_add_loss_device: detect.m:135's qp.ub = qp.ub + Cneg * max(1 + score, 0) for the records of a payload, the quantity
 *   that decides whether mining re-optimises (detect.m:148-152).  Over the m = min(max(word 0, 0), capacity) records PRESENT in
 *   d_payload -- whether pbd_qp_add_device wrote them into the cache or dropped them for lack of room, as detect.m:133-136 counts
 *   them -- ub = ub + Cl * R(h) with h_j = max(0, 1 - y * score_j) in double, score_j = record j's float score widened, y = +1
 *   and Cl = Cpos when label > 0, else y = -1 and Cl = Cneg, and R the reduction above with record j on lane j mod
 *   PBD_QP_LANES.  *added (may be NULL) receives the addend Cl * R(h).  PBD_ERR_STATE while ub is NaN (no pbd_qp_opt /
 *   pbd_qp_one since create or clear).  The records are those of the handle the QP was created from (its record stride).  The
 *   call runs on the QP's stream; a QP on the stream of the handle it was created from is thereby ordered behind the payload's
 *   producer, a QP on another stream waits for the device first (the call does not name the producing handle).
 * Every call is synchronous.  Errors: PBD_ERR_INVALID for bad arguments, PBD_ERR_STATE for an empty cache or pass set; the
 * message is pbd_qp_last_error(q). */
#define PBD_QP_LANES 1024
typedef struct pbd_qp pbd_qp;
struct pbd_qp_config {
    int capacity;
    double C, wpos;               /* 0: 0.002, 2 */
    void *stream;                 /* hipStream_t or NULL */
    const double *wreg, *w0;      /* [model vector length] or NULL */
    const int32_t *noneg;         /* [nnoneg] or NULL */
    int nnoneg;
};
struct pbd_qp_info {
    int n, nsv, nfix, capacity, len, hdr_words, values;   /* entries, support vectors, fixed, strides of an entry */
    double lb, ub, loss, l;
    int lb_dropped, passes, converged, pad;
};
int pbd_qp_create(const pbd_handle *h, const struct pbd_qp_config *cfg, pbd_qp **out);
void pbd_qp_destroy(pbd_qp *q);
const char *pbd_qp_last_error(const pbd_qp *q);   /* q NULL: the last failed pbd_qp_create of this thread */
int pbd_qp_add(pbd_qp *q, const pbd_handle *h, int n, const int32_t *hdr, const void *values, const int32_t *ids, int *taken);
int pbd_qp_add_device(pbd_qp *q, pbd_handle *h, const int32_t *d_payload, int capacity, const int32_t *d_hdr, const void *d_values,
                      int label, int id_base, int32_t *d_taken);
int pbd_qp_fix(pbd_qp *q);
int pbd_qp_clear(pbd_qp *q);
int pbd_qp_add_loss_device(pbd_qp *q, const int32_t *d_payload, int capacity, int label, double *added);
int pbd_qp_prune(pbd_qp *q, int *n);
int pbd_qp_one(pbd_qp *q, const int32_t *order, int norder, uint64_t seed, struct pbd_qp_info *state);
int pbd_qp_opt(pbd_qp *q, double tol, int iter, uint64_t seed, struct pbd_qp_info *state);
int pbd_qp_weights(pbd_qp *q, double *w);
int pbd_qp_apply(pbd_qp *q, pbd_handle *h);   /* the in-place model update from the QP's weights: see pbd_set_model_vector */
int pbd_qp_scores(pbd_qp *q, double *s, int *n);
int pbd_qp_state(pbd_qp *q, struct pbd_qp_info *state, double *a, uint8_t *sv, double *w);
int pbd_qp_entries(pbd_qp *q, int first, int count, int32_t *hdr, float *values, double *b, double *d, int32_t *ids);

/* ---- part types of a flexible-mixtures model (new surface): clusterparts.m + k_means.m of the reference's Matlab training
 * code (matlab/learning), and the anchors of buildmodel.m:68-70.  For each of nparts parts, `trials` independent k-means runs
 * over the npos positives' offsets to the parent; the run with the smallest sum of distances gives the part's types.
 * The handle supplies the stream, the workspace and the error text; nothing of its model is read.  All arithmetic is double,
 * whatever the handle's T.  Matlab's rand is not reproduced: the starting points are splitmix64 draws (below), and the defined
 * behaviour is partsbaseddetector_amd/trainmodel.py's cluster_parts_ref, which the device matches bit for bit.
 * def: double[nparts][npos][2], each part's (x, y) per positive (data_def.m).  parent (HOST memory in both forms): 0-based,
 * parent[0] = -1 (the root), 0 <= parent[p] < p for every other part.  K (HOST memory in both forms): the types of each part,
 * 1..16.  PBD_ERR_INVALID: nparts < 2, npos < 1, trials < 1, max_iter < 1, nparts * trials above 2^20, a K outside 1..16, a
 * parent table that breaks the order above.
 * Data: X[n] = def[p][n] - def[parent[p]][n] per coordinate; for the root X[n] = def[c][n] - def[0][n] with c its
 *   lowest-numbered child (clusterparts.m:9-14).
 * Start of trial r of part p: centroid t = X[z mod npos], z = splitmix64 output number (p * trials + r) * 16 + t (0-based) of
 *   partsbaseddetector_amd/synth.py's splitmix64(seed, nparts * trials * 16).  Draws may repeat, as ceil(rand * n) may.
 * One iteration: D_t(n) = (0.0 + dx * dx) + dy * dy with dx = X[n].x - c_t.x, dy likewise, each operation rounded on its own.
 *   The label of n is the first t whose D_t(n) is not NaN and is strictly below every earlier one (Matlab's min: NaN is skipped,
 *   the first minimum wins) and z(n) that distance; a point whose distances are all NaN gets label 0 and z = NaN.  Then
 *   c_t = R(x of the members) / count_t and likewise for y, R the reduction stated with the QP above (point n on lane n mod
 *   PBD_QP_LANES, a point that is not a member adds nothing); a cluster without members gets a NaN centroid, so it never wins a
 *   point again.
 * End of a trial: labels start at -1, so the first iteration always changes one; the trial ends after the first iteration that
 *   changes no label, or after max_iter iterations.  sumdist = R(z) of the last iteration.
 * Pick (clusterparts.m:25-26): the first trial whose sumdist is not NaN and strictly below every earlier one; none: trial 0.
 *   idx (0-based types), centres and counts are that trial's; centres of unused (t >= K) or empty types are NaN, their counts 0.
 * Anchors (buildmodel.m:68-70, then zeroIndex): a type's centre is the mean of def[child] - def[parent] over its members, so
 *   anchor = matlab_round(centre + 1.0) - 1 per coordinate, rounding halves away from zero (a centre of exactly -0.5 gives 0,
 *   not round(-0.5) = -1), saturating at the int32 range.  The root's anchors and those of NaN centres are 0.
 * Defined differently from the reference, on purpose: a type with one member keeps that member as its centre (Matlab's mean of
 *   a 1 x 2 row collapses it to (x + y) / 2 in both coordinates), and max_iter exists.
 * info[p]: the picked trial, its iterations and its sumdist.  sumdist_all / iters_all ([nparts][trials], either may be NULL):
 *   every trial's.  pbd_cluster_parts is synchronous and takes host pointers; pbd_cluster_parts_device takes device pointers
 *   (def and every output; parent and K stay on the host), is asynchronous on pbd_stream() and reads def in place.
 * PBD_ERR_STATE while a batch is in flight.  pbd_cluster_parts* leave the resident detect result alone. */
struct pbd_cluster_info {
    int32_t best_trial, iterations;
    double sumdist;
};
int pbd_cluster_parts(pbd_handle *h, int nparts, int npos, const double *def, const int32_t *parent, const int32_t *K, int trials,
                      int max_iter, uint64_t seed, int32_t *idx, double *centres, int32_t *counts, int32_t *anchors,
                      struct pbd_cluster_info *info, double *sumdist_all, int32_t *iters_all);
int pbd_cluster_parts_device(pbd_handle *h, int nparts, int npos, const double *d_def, const int32_t *parent, const int32_t *K,
                             int trials, int max_iter, uint64_t seed, int32_t *d_idx, double *d_centres, int32_t *d_counts,
                             int32_t *d_anchors, struct pbd_cluster_info *d_info, double *d_sumdist_all, int32_t *d_iters_all);

/* ---- IConvolutionEngine (include/IConvolutionEngine.hpp:44-68), SpatialConvolutionEngine. */
/* setFilters(filters): filters[f] is ksize[f] x (ksize[f]*flen) values of T.  pbd_create already
 * installs the model's filters; this replaces them (src/SpatialConvolutionEngine.cpp:133-159). */
int pbd_conv_set_filters(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize);
/* pdf(features, responses): resp[l] receives nfilters planes of rows[l] x cols[l]
 * (responses[l][f] at resp[l] + f*rows[l]*cols[l]) (src/SpatialConvolutionEngine.cpp:106-124). */
int pbd_conv_pdf(pbd_handle *h, int nlevels, const void *const *feat, const int *rows, const int *cols,
                 void *const *resp);

/* ---- DynamicProgram<T> (include/DynamicProgram.hpp:74-75). */
int pbd_num_ptr_slots(const pbd_handle *h);   /* back-pointer maps per (level): sum over non-root parts of parent mixtures */
int pbd_ptr_slot(const pbd_handle *h, int component, int part); /* slot of (part, parent mixture 0) */
/* min(parts, scores, Ix, Iy, Ik, rootv, rooti) (src/DynamicProgram.cpp:67-173).
 * resp[l]: nfilters planes; Ix/Iy/Ik[l]: pbd_num_ptr_slots planes of int32 (plane slot(part)+m =
 * reference Ix[l][c][part][m]); rootv[l]/rooti[l]: ncomponents planes.
 *
 * Non-finite scores.  Every intersection z the distance transform's forward scan pushes is the reference's, in every kernel
 * variant: a NaN z (from Inf - Inf: two neighbouring equal infinities along a line; or from a NaN score) is pushed, and since
 * s <= NaN is false nothing beneath it is popped again.
 *   1. +-Inf and NaN scores are accepted here, and the fp16 responses of PBD_CONV_MFMA_F16 / _F16_ANY that saturated to +-inf are
 *      accepted by the detect path; nothing is refused.
 *   2. While NO NaN intersection forms anywhere in the dynamic program (isolated -Inf cells in lines that keep a finite cell,
 *      isolated +Inf cells, saturated fp16 responses of that shape), every output -- Ix, Iy, Ik, rootv, rooti -- equals the
 *      reference's bit for bit, under every launch choice.
 *   3. Where a NaN intersection forms (a masked REGION of -Inf, neighbouring +Inf, NaN scores), the read-out of position q takes
 *      entry max{k : z[k] < os + q} of the line's envelope, a comparison with NaN being false.  This is a decision of this
 *      library, not the reference's answer: the reference's loop walks up from entry 0 ("while (z[k+1] < os) k++") and stops
 *      below the first NaN whatever lies above it, an artefact of the direction of that loop; walking down from the top finds
 *      the entries above the NaN that do cover q.  Every kernel variant gives this one answer, so a plane gives the same
 *      pointers alone and in a batch.  NaN values in rootv stand at the same places on every path; their sign and payload are
 *      unspecified.  Where rule 2 applies, rule 3 selects the reference's entry.
 * To mask a region and stay within rule 2, use a large finite negative score as pbd_detect_latent does (-1e10). */
int pbd_dp_min(pbd_handle *h, int nlevels, const int *rows, const int *cols, const void *const *resp,
               int32_t *const *Ix, int32_t *const *Iy, int32_t *const *Ik, void *const *rootv,
               int32_t *const *rooti);
/* argmin(parts, rootv, rooti, scales, Ix, Iy, Ik, candidates) (src/DynamicProgram.cpp:190-255) on
 * the device-resident result of the last pbd_dp_min / pbd_detect*.  Candidates are written sorted by
 * (frame, level, component, root_y, root_x): the raster order of the reference's Math::find per (level, component)
 * (:208-216); its order ACROSS levels is nondeterministic (#pragma omp critical, :246-251).  The order is produced on the
 * device (ordered compaction, no sort); when more than `capacity` are found, the first `capacity` of that order are
 * returned with PBD_ERR_CAPACITY.  PBD_ERR_STATE without one: none yet, after pbd_features_pyramid, pbd_conv_pdf, pbd_conv_set_filters,
 * a model update, pbd_warp_positives, pbd_detect_latent or a mixed-size call. */
int pbd_dp_argmin(pbd_handle *h, const float *scales, int32_t *cand, int capacity, int *ncand);

/* ---- PartsBasedDetector<T>::detect (include/PartsBasedDetector.hpp:172-173, src/PartsBasedDetector.cpp:69-95).
 * `depth` of the 3-argument overload has no parameter here: the reference ignores it (:91-93), and the opt-in filter it leaves
 * commented out is pbd_depth_consistency, chained by the callers' detect(im, depth) when they turn it on; the callers' later use of
 * the depth image, Candidate::boundingBox3D, is pbd_boxes3d (next to pbd_set_nms). */
int pbd_detect(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes,
               int32_t *cand, int capacity, int *ncand);
/* The same for an image of any accepted depth (depth_code as in pbd_features_pyramid); pbd_detect is depth_code 0.
 * The equal-size batch entry points take 8-bit frames; pbd_detect_frames* (below) take every depth. */
int pbd_detect_typed(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes,
                     int depth_code, int32_t *cand, int capacity, int *ncand);
/* New surface (the reference has no batch API): nframes equally-sized frames, results identical to
 * nframes pbd_detect calls, candidate `frame` field = index in the batch. */
int pbd_detect_batch(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                     size_t stride_bytes, int32_t *cand, int capacity, int *ncand);
/* Pipelined form of pbd_detect_batch (new surface, as the batch API): submit() copies the frames into a pinned
 * staging buffer of the handle, starts their transfer on a copy stream and enqueues the whole path behind it, without
 * waiting; wait() returns the candidates of the oldest submitted batch (same records and order as pbd_detect_batch).
 * Up to two batches may be in flight -- submit(k+1), then wait(k) -- so that the host-side staging and the PCIe
 * transfer of batch k+1 overlap the kernels of batch k.  The synchronous entry points and the staged read-back
 * refuse to run (PBD_ERR_STATE) while a batch is in flight.
 * pbd_detect_batch_wait releases the oldest batch's slot on EVERY return except the refusals that look at no batch: "no
 * batch in flight" (PBD_ERR_STATE) and a null handle, cand or ncand (PBD_ERR_INVALID).  In particular a wait that returns
 * PBD_ERR_CAPACITY -- more candidates than `capacity` or than pbd_config.max_candidates: the first min(capacity, max_candidates)
 * records are delivered and counted in *ncand; or, with pbd_set_nms on, more than max_candidates before the suppression: *ncand = 0 -- has
 * consumed its batch: the next wait returns the NEXT batch, and a caller that wants the rest of the list has to submit the
 * frames again.  A caller that keeps a count of batches in flight (detector.DetectorPool, pbdhost::FrameStream) therefore
 * counts a failed wait as a collected batch.  A refused submit enqueues nothing and leaves the batches in flight as they were.
 * A submit replaces the resident result where it enqueues.  After the last wait the resident result is that of the batch submitted last
 * (the staged read-back, pbd_examples*, pbd_argmin_device_out and the rest read it as after pbd_detect_batch of those frames). */
int pbd_detect_batch_submit(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                            size_t stride_bytes);
int pbd_detect_batch_wait(pbd_handle *h, int32_t *cand, int capacity, int *ncand);
/* submit() for frames already resident in device memory (d_frames as in pbd_detect_batch_device; they must stay
 * untouched until the matching wait() returns): nothing is copied in, the candidates' read-back of batch k overlaps the
 * kernels of batch k+1. */
int pbd_detect_batch_device_submit(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels);
/* Same, frames already resident in device memory: d_frames = nframes contiguous rows*cols*channels
 * images.  cand is a HOST buffer. */
int pbd_detect_batch_device(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                            int32_t *cand, int capacity, int *ncand);

/* Device-resident output (new surface: multi-GPU jobs, device pipelines).  The candidate list stays on the device in the
 * caller's buffer d_payload = int32[1 + capacity * pbd_candidate_stride()] ("payload"):
 *   word 0      number of candidates FOUND -- may exceed `capacity`; then only the first `capacity` of the order are present
 *   word 1...   min(found, capacity) records, sorted by (frame, level, component, root_y, root_x); `frame` = frame_offset +
 *               index in the batch (frames sharded over GPUs: the global frame id)
 * i.e. exactly what a rank contributes to the one gather of Candidate lists per batch (partsbaseddetector_amd/dist.py hands
 * this buffer to all_gather_into_tensor as it is; nothing passes through the host).  ASYNCHRONOUS: the call returns once
 * the work is enqueued on pbd_stream(); order later work behind that stream (or call pbd_synchronize).
 * pbd_argmin_device_out re-emits the list of the batch still resident from the last pbd_detect* call -- used after a
 * capacity overflow (word 0 > capacity) with a larger buffer; the dynamic program is not run again.
 * PBD_ERR_STATE without such a batch: none yet, or the last writer was one of the staged calls (pbd_features_pyramid, pbd_conv_pdf,
 * pbd_dp_min), pbd_conv_set_filters, a model update, pbd_warp_positives or pbd_detect_latent. */
int pbd_detect_batch_device_out(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                                int frame_offset, int32_t *d_payload, int capacity);
int pbd_argmin_device_out(pbd_handle *h, int frame_offset, int32_t *d_payload, int capacity);
/* the hipStream_t every kernel of this handle runs on (pbd_config.stream, or the library's own) */
void *pbd_stream(const pbd_handle *h);

/* ---- frames of different sizes in one call (new surface, as the batch API).
 * A frame: `data` is a host pointer (pbd_detect_frames) or a device pointer (the _device forms), rows x cols pixels of
 * `channels` interleaved values of the call's depth, rows `stride_bytes` apart (>= cols * channels * element size).  A
 * _device frame may be a REGION of a larger device image -- its first pixel, and that image's pitch as stride_bytes: it is
 * read in place, without a copy, and gives what pbd_detect gives on the cropped image (boxes in the region's coordinates).
 * A _device frame's pointer and stride_bytes are multiples of the element size (2, 4 or 8 bytes for 16U / 32F / 64F).
 * Result: exactly the records of nframes separate pbd_detect_typed calls, one per frame, concatenated; `frame` = index in the
 * call (+ frame_offset for _device_out), order (frame, level, component, root_y, root_x), `level` = level of that frame's own
 * pyramid.  One `channels` (1 or 3) and one depth_code (as pbd_features_pyramid; all four for every form) per call.
 * nframes <= max_batch, PBD_ERR_CAPACITY, payload word 0, pbd_set_nms (each frame within its own Rect(0, 0, cols, rows)) and
 * the NaN / Inf refusal of host 32F / 64F frames (naming the frame) behave as in the batch calls above.  A frame too small to
 * plan or with a pitch below its row size is PBD_ERR_INVALID, naming its index, before anything is enqueued.  With level
 * sharding on (world > 1): PBD_ERR_UNSUPPORTED; while a batch is in flight: PBD_ERR_STATE.
 * After a mixed call, pbd_get_stage / pbd_get_pyramid_image address (frame in the call, level of that frame's pyramid),
 * pbd_argmin_device_out re-emits the mixed list, and pbd_dp_argmin (DynamicProgram::argmin over ONE image's scales) returns
 * PBD_ERR_STATE.  There is no pipelined _submit / _wait form for mixed frames. */
typedef struct pbd_frame {
    const void *data;
    int rows, cols;
    size_t stride_bytes;
} pbd_frame;
int pbd_detect_frames(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code,
                      int32_t *cand, int capacity, int *ncand);
/* the same for frames in device memory; cand is a HOST buffer */
int pbd_detect_frames_device(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code,
                             int32_t *cand, int capacity, int *ncand);
/* the same with the list left on the device in the caller's payload, asynchronous (as pbd_detect_batch_device_out) */
int pbd_detect_frames_device_out(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code,
                                 int frame_offset, int32_t *d_payload, int capacity);

/* ---- staged read-back of the last pbd_detect* or pbd_detect_latent call (tests, profiling) ----
 * A stage is readable only if the last computation produced it: after pbd_conv_set_filters the responses and DP
 * results are gone, and after pbd_dp_min (which starts from uploaded responses) PBD_STAGE_FEATURES is PBD_ERR_STATE.
 * After pbd_features_pyramid only PBD_STAGE_FEATURES and the level images are readable (the responses and DP results of an
 * earlier call are gone); after pbd_conv_pdf PBD_STAGE_FEATURES (the uploaded maps) and PBD_STAGE_RESPONSES.
 * After pbd_detect_latent the stages are those of its masked run (see there), whose responses have one plane per
 * (component, part, mixture), not per filter; after a model update or pbd_conv_set_filters nothing of a latent result is readable
 * (pbd_get_stage, pbd_examples* and pbd_part_scores* give PBD_ERR_STATE: its features live in the twin with everything else).
 * Frames and levels are those of the last call alone: an address an earlier, larger result had is PBD_ERR_INVALID, and
 * pbd_get_stage looks at the address before it looks at the stage (a bad address of a stage that is not held is PBD_ERR_INVALID).
 * A refused call leaves the previous result readable. */
enum { PBD_STAGE_FEATURES = 0, PBD_STAGE_RESPONSES = 1, PBD_STAGE_ROOTV = 2, PBD_STAGE_ROOTI = 3 };
int pbd_get_stage(pbd_handle *h, int stage, int frame, int level, void *dst, size_t dst_bytes);

/* ---- per-kernel timing with HIP events on the library's stream (bench.py roofline) ---- */
enum { PBD_K_RESIZE = 0, PBD_K_PYRDOWN, PBD_K_HOG_HIST, PBD_K_HOG_FEAT, PBD_K_CONV, PBD_K_DT_ROWS,
       PBD_K_DT_COLS, PBD_K_DP_COMBINE, PBD_K_DP_ROOT, PBD_K_ARGMIN,
       /* pbd_boxes3d_camera*, pbd_cluster_objects*; k_cl_crop_scan / k_cl_grid_scan time the three k_scan_* kernels of that scan */
       PBD_K_CAMERA_BOXES, PBD_K_CL_CROP_COUNT, PBD_K_CL_CROP_SCAN, PBD_K_CL_CROP_SCATTER, PBD_K_CL_CLEAR, PBD_K_CL_GRID_COUNT,
       PBD_K_CL_GRID_SCAN, PBD_K_CL_GRID_SCATTER, PBD_K_CL_HOOK, PBD_K_CL_LABEL, PBD_K_CL_BEST, PBD_K_CL_SELECT, PBD_K_CL_OUT,
       /* pbd_depth_consistency*; k_dc_select times its three size classes, k_dc_compact the decision and the compaction */
       PBD_K_DC_CLASSIFY, PBD_K_DC_SELECT, PBD_K_DC_COMPACT,
       /* pbd_candidate_mask* (k_mk_hull times k_mk_init and k_mk_hull), pbd_part_poses* */
       PBD_K_MK_HULL, PBD_K_MK_TILE, PBD_K_PART_POSES,
       /* pbd_examples*: the walk of every record, then the gather of its feature windows */
       PBD_K_EX_WALK, PBD_K_EX_GATHER,
       /* the training QP (pbd_qp_*): named for traces; a pbd_qp has no profile and a handle's profile does not see them */
       PBD_K_QP_WRITE, PBD_K_QP_SCORE, PBD_K_QP_PASS, PBD_K_QP_LINCOMB, PBD_K_QP_SLOTS, PBD_K_QP_NORM, PBD_K_QP_WRAW,
       PBD_K_QP_GATHER,
       /* pbd_warp_positives*: the patches of the kept boxes, then every box's example (the HOG of the patches is timed under
          k_hog_hist / k_hog_feat) */
       PBD_K_WARP, PBD_K_WARP_EMIT,
       /* pbd_part_nms* (k_ev_nms_select times the check, the cut and the pick ranks), pbd_best_overlap*, pbd_eval_pck*,
          pbd_eval_apk* (k_ev_apk_rank times the keys and the order) */
       PBD_K_EV_NMS_SELECT, PBD_K_EV_NMS_PAIRS, PBD_K_EV_NMS_GREEDY, PBD_K_EV_NMS_EMIT, PBD_K_EV_BEST, PBD_K_EV_PCK,
       PBD_K_EV_APK_RANK, PBD_K_EV_APK_CLOSE, PBD_K_EV_APK_AP,
       /* pbd_qp_add_loss_device (named for traces, as the other QP kernels) */
       PBD_K_QP_HINGE,
       /* pbd_cluster_parts*: every (part, trial)'s k-means run, then the pick per part */
       PBD_K_KM_TRIALS, PBD_K_KM_PICK,
       /* pbd_grid_nms* / pbd_set_root_nms: the grid maxima of a set of planes */
       PBD_K_GRID_NMS,
       /* pbd_top_k_cells* / pbd_set_top_k / pbd_top_k*: the K best elements of every segment, or records of every frame */
       PBD_K_TOP_K,
       /* pbd_set_depth_prune / pbd_depth_prune*: the plausibility test of the root cells, or of a list's records */
       PBD_K_DEPTH_PRUNE,
       /* pbd_max_marginals: the forward transforms re-run for the messages and the mirrored transforms (the detect path's
          transform kernels, counted here and not under k_dt_rows / k_dt_cols), the messages, the contexts, the reduction over the
          parent's types; pbd_marginal_poses*: the decode */
       PBD_K_MM_DT_ROWS, PBD_K_MM_DT_COLS, PBD_K_MM_MESSAGES, PBD_K_MM_CONTEXT, PBD_K_MM_DOWN, PBD_K_MM_DECODE,
       /* pbd_set_scale_nms / pbd_scale_nms*: the scale-space maxima of the root cells, or of a list's records */
       PBD_K_SCALE_NMS,
       PBD_K_COUNT };
/* on = 1: every kernel launch carries a start / stop event pair (the runtime isolates a timed dispatch: about 1 ms per
 * 64-frame step of ~45 launches); on = 2: only the convolution (one launch per step: free); 0: off */
int pbd_profile_enable(pbd_handle *h, int on);
int pbd_profile_reset(pbd_handle *h);
/* total_ms / launches accumulated since the last reset for kernel id k */
int pbd_profile_read(pbd_handle *h, int k, double *total_ms, int *launches);
const char *pbd_kernel_name(int k);
int pbd_synchronize(pbd_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* PBD_H_ */
