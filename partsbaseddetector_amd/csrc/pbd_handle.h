// pbd_handle.h -- private to the C entry layer (pbd_capi*.hip), not installed: the owners of the handle's HIP resources, plans,
// struct pbd_handle, and the layer every entry point is written on (status codes and messages, the ABI guard, staged tables,
// workspace carving, profiling scopes).
#pragma once
#include "pbd_internal.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <numeric>
#include <new>
#include <set>
#include <stdexcept>
#include <type_traits>
#include <utility>

#pragma GCC visibility push(hidden)   // nothing declared here is part of the library's ABI

namespace pbd {

// Move-only owner of one HIP resource: device memory (Free = hipFree), pinned host memory (hipHostFree), an event or a
// stream.  `size` is the bytes or elements held (memory only).  The destructor frees the resource and ignores HIP errors:
// nothing is left to report them to.
template <typename T, auto Free>
struct Owned {
    T *p = nullptr;
    size_t size = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept { swap(o); }
    Owned &operator=(Owned o) noexcept { swap(o); return *this; }   // `o` takes the old resource away and frees it
    ~Owned() { if (p) (void)Free(p); }
    void swap(Owned &o) noexcept { std::swap(p, o.p); std::swap(size, o.size); }
};
using Event = Owned<std::remove_pointer_t<hipEvent_t>, hipEventDestroy>;

struct DevBuf : Owned<void, hipFree> {   // grow-only device workspace; growing does not keep the contents
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= size) return hipSuccess;
        *this = DevBuf{};
        const size_t want = bytes + bytes / 8 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) size = want;
        return e;
    }
    // exactly `bytes` (at least 16), whatever was held before: for buffers of gigabytes, where ensure()'s eighth on top matters
    hipError_t alloc_exact(size_t bytes)
    {
        *this = DevBuf{};
        const size_t want = std::max<size_t>(bytes, 16);
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) size = want;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct HostBuf : Owned<void, hipHostFree> {   // grow-only pinned host memory: below `bytes`, reallocated to `want`
    hipError_t ensure(size_t bytes, size_t want)
    {
        if (bytes <= size) return hipSuccess;
        *this = HostBuf{};
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) size = want;
        return e;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// A small table on its way to the device through pinned staging memory, which is rewritten only once its previous copy has
// completed.  One per stage: a table shared between stages would make one stage's call wait for another's copy.
struct StagedTable {
    HostBuf host;
    DevBuf dev;
    Event copied;
    int stage(pbd_handle *h, const void *src, size_t bytes);   // PBD_OK or the failure's status code; on the handle's stream
    template <typename T> T *as() const { return dev.as<T>(); }
};

// Lays the pieces of a buffer out one after another, each starting at the next multiple of `align` bytes.  Without a base it
// only adds up (the sizing pass); with one it also hands out the pieces' addresses (the carving pass).  A stage describes its
// pieces once, in a function run for both passes (carve() below).  `sizes[0..nsizes)`, when set, receive the pieces' sizes.
struct Carve {
    uint8_t *base = nullptr;
    size_t off = 0;
    int pieces = 0;
    long long *sizes = nullptr;
    int nsizes = 0;
    static size_t up(size_t v, size_t align) { return (v + align - 1) / align * align; }
    template <typename T> T *take(size_t bytes, size_t align = 256)
    {
        off = up(off, align);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += bytes;
        if (pieces < nsizes) sizes[pieces] = (long long)bytes;
        ++pieces;
        return p;
    }
};

template <typename T>
struct DevTable : Owned<T, hipFree> {   // small immutable table uploaded once; `size` elements
    hipError_t upload(const std::vector<T> &h)
    {
        *this = DevTable{};
        if (h.empty()) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&this->p), h.size() * sizeof(T));
        if (e != hipSuccess) return e;
        this->size = h.size();
        return hipMemcpy(this->p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// A stream created here (and destroyed with its owner), or one borrowed from the caller (pbd_config.stream)
struct Stream {
    Owned<std::remove_pointer_t<hipStream_t>, hipStreamDestroy> own;   // null when borrowed
    hipStream_t s = nullptr;
    hipError_t create()
    {
        const hipError_t e = hipStreamCreateWithFlags(&own.p, hipStreamNonBlocking);
        s = own.p;
        return e;
    }
    void borrow(hipStream_t b) { s = b; }
    operator hipStream_t() const { return s; }
};

struct Plan {
    // key
    int kind = 0;   // 0: from image size, 1: from explicit feature-map sizes, 2: mixed sizes (below), 3: a group of a mixed plan's
                    // frames for the dynamic program, 4: only the suppression's canvas tables of a list of frame sizes (pbd_suppress*)
    int rows = 0, cols = 0;         // the geometry does not depend on the channel count (offsets are in pixels)
    std::vector<int> key_dims;
    // geometry
    int nlevels = 0;
    std::vector<LevelDesc> lv;
    std::vector<float> scales;
    long long pix_per_frame = 0, blk_per_frame = 0, cell_per_frame = 0, npix_resized = 0, quad_per_frame = 0;
    int interval = 0;
    int nrows_flat = 0, ncols_flat = 0;
    bool ptr8 = false;              // no feature map side exceeds 256: positions fit uint8 (back-pointer planes at half the bytes)
    int longest = 0;                // longest side of any feature map of the plan (rows / columns of the distance transform)
    bool padded = false;            // built under a non-zero pbd_set_padding: its levels carry the pad (LevelDesc::padx / pady)
    int nfine = 0;                  // image plans: the levels of the fine octave, which come first (pbd_set_fine_octave); lv[nfine] is
                                    // the reference's level 0
    bool fine = false;              // some level's bin size is not the model's (LevelDesc::sbin): the HOG stage runs per hgroups
    std::vector<HogGroup> hgroups;  // the runs of consecutive levels of one bin size (finish_plan_tables)
    int ntiles = 0;
    // device tables
    DevTable<LevelDesc> d_lv;
    DevTable<LevelDesc> d_lv_img;   // fine plans: the reference levels alone, every level image once (pass 1 of the two-pass HOG)
    int nlv_img = 0;
    DevTable<ResizeTabX> d_tabx;
    DevTable<ResizeTabY> d_taby;
    DevTable<ResizeTabXf> d_tabxf;   // the same mapping with float coefficients (16U / 32F / 64F images)
    DevTable<ResizeTabYf> d_tabyf;
    DevTable<ConvTile> d_tiles, d_shaped, d_htiles;
    int nshaped[3] = {0, 0, 0}, nhtiles = 0;
    // strip-sequence tiles of the exact 5 x 5 convolution, per number of frames in a launch (built on first use)
    std::map<int, DevTable<ConvSegTile>> segtiles;
    DevTable<int> d_row2level, d_rowoff, d_col2level, d_coloff;
    DevTable<long long> d_stk_row_off, d_stk_col_off;
    long long stk_per_jf = 0;
    DevTable<float> d_scales;
    // host copies of the resize tables (image plans): mixed plans are assembled from them
    std::vector<ResizeTabX> htabx;
    std::vector<ResizeTabY> htaby;
    std::vector<ResizeTabXf> htabxf;
    std::vector<ResizeTabYf> htabyf;

    // ---- kind 2: a mixed-size call planned as ONE virtual frame whose level table is the frames' own pyramids, concatenated
    // frame-major (key_dims = rows, cols of every frame in call order).  Every stage after the pyramid runs over it unchanged.
    int mixed_frames = 0;
    std::vector<int> lv_frame, lv_local;    // per virtual level: frame of the call, level of that frame's pyramid
    std::vector<int> frame_lv0;             // [mixed_frames + 1] first virtual level of each frame
    std::vector<int> frame_nfine;           // [mixed_frames] fine levels at the head of each frame's levels
    DevTable<int> d_lv_frame, d_lv_local;
    // pyramid launches: launch 0 = every frame's resized levels, launch k >= 1 = octave k of every frame; launch k's levels are
    // run_lev[lev0[k] ..], its n[k] + 1 pixel offsets run_off[off0[k] ..]
    std::vector<int> run_lev, run_lev0, run_n;
    std::vector<long long> run_off, run_off0, run_npix;
    DevTable<int> d_run_lev;
    DevTable<long long> d_run_off;
    // post-processing: per frame {rows, cols}, global-canvas word offset; the frames of each canvas kind
    std::vector<int2> fdim;
    std::vector<long long> fcanvas;
    std::vector<int> post_lds, post_glb;
    size_t post_lds_words = 0, post_glb_words = 0;
    DevTable<int2> d_fdim;
    DevTable<long long> d_fcanvas;
    DevTable<int> d_post_lds, d_post_glb;
    DevTable<int> d_frame_lv0;              // frame_lv0 on the device (pbd_examples*, uploaded on first use)
    // pbd_set_root_nms: the (level, component) planes of one frame's rootv cut into blocks of gn_sz + 1 (rebuilt when sz changes)
    int gn_sz = 0;
    long long gn_blocks = 0;
    DevTable<GnPlane> d_gn;
    // pbd_set_top_k on a mixed plan: the frames' ranges of the virtual frame's root cells as segments (built on first use)
    long long tk_tiles = 0;
    DevTable<TopKTab> d_tk;
    // dynamic program in groups of whole frames when the virtual frame's scratch exceeds the budget: sub-plans whose cell
    // offsets start at 0 (cell0 = the group's first cell in the virtual frame), built for `chunk_budget`
    size_t chunk_budget = 0;
    std::vector<std::unique_ptr<Plan>> chunk_plans;
    std::vector<long long> chunk_cell0;
};

// cv::resize INTER_LINEAR coefficient tables of one axis (OpenCV imgwarp.cpp), appended to `fix` (8-bit
// fixed point) and `flt` (16U / 32F / 64F): destination index 0..dst-1 from a source of `src` elements.  Columns: the first tap
// sx (the second is sx + 1; `last`: sx is the last source column and the only tap); rows: the two taps, clamped to the source.
// The resized pyramid levels and the warped positives' patches are built from these and nothing else.
inline short sat_short_round(float v)
{
    long iv = lrint((double)v);
    return (short)(iv < -32768 ? -32768 : iv > 32767 ? 32767 : iv);
}
inline void resize_taps_x(int src, int dst, std::vector<ResizeTabX> &fix, std::vector<ResizeTabXf> &flt)
{
    const double scale_x = 1. / ((double)dst / src);
    for (int dx = 0; dx < dst; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0; sx = 0; }
        const int last = sx >= src - 1;
        if (last) { fx = 0; sx = src - 1; }
        fix.push_back({sx, sat_short_round((1.f - fx) * 2048), sat_short_round(fx * 2048)});
        flt.push_back({sx, last, 1.f - fx, fx});
    }
}
inline void resize_taps_y(int src, int dst, std::vector<ResizeTabY> &fix, std::vector<ResizeTabYf> &flt)
{
    const double scale_y = 1. / ((double)dst / src);
    for (int dy = 0; dy < dst; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int y0 = std::min(std::max(sy, 0), src - 1), y1 = std::min(std::max(sy + 1, 0), src - 1);
        fix.push_back({y0, y1, sat_short_round((1.f - fy) * 2048), sat_short_round(fy * 2048)});
        flt.push_back({y0, y1, 1.f - fy, fy});
    }
}

struct Group {   // DT jobs of the parts of one tree depth + combine jobs of their parents
    std::vector<DtJob> jobs;
    std::vector<ChildDesc> childs;
    std::vector<CombineJob> cjobs;
    std::vector<SeqCombineJob> sjobs;     // sequential schedule (shared filter ids): replaces childs / cjobs
    DevTable<DtJob> d_jobs;
    int bz_x = 0, bz_y = 0;               // all jobs: linear coefficient exactly -0.0 and a != 0 (DpParams::bz_x / bz_y)
    DevTable<ChildDesc> d_childs;
    DevTable<CombineJob> d_cjobs;
    DevTable<SeqCombineJob> d_sjobs;
};

// Quadratic(-w0, -w1), Quadratic(-w2, -w3) of a deformation's four float32 values (-(+0.0f) is -0.0)
inline void set_quadratics(DtJob &j, const float *w)
{
    j.ax = (double)(-w[0]); j.bx = (double)(-w[1]); j.ay = (double)(-w[2]); j.by = (double)(-w[3]);
}
// the usual deformation (w1 = w3 = +0.0f, so b = -0.0): the group's passes then run without the b terms
inline void set_variant_flags(Group &g)
{
    auto neg_zero = [](double v) { return v == 0.0 && std::signbit(v); };
    g.bz_x = g.bz_y = 1;
    for (const DtJob &j : g.jobs) {
        if (!(neg_zero(j.bx) && j.ax != 0.0)) g.bz_x = 0;
        if (!(neg_zero(j.by) && j.ay != 0.0)) g.bz_y = 0;
    }
}

struct Prof {
    int on = 0;                      // 0: off, 1: every kernel, 2: the convolution only (pbd_profile_enable)
    struct Rec { int k; Event a, b; };
    std::vector<Rec> recs;
    std::vector<Event> pool;
    double total[PBD_K_COUNT] = {0};
    int launches[PBD_K_COUNT] = {0};
    Event get()
    {
        Event e;
        if (pool.empty()) { (void)hipEventCreate(&e.p); return e; }
        e = std::move(pool.back());
        pool.pop_back();
        return e;
    }
    void flush()
    {
        for (auto &r : recs) {
            (void)hipEventSynchronize(r.b.p);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a.p, r.b.p) == hipSuccess) { total[r.k] += ms; launches[r.k] += 1; }
            pool.push_back(std::move(r.a)); pool.push_back(std::move(r.b));
        }
        recs.clear();
    }
};

// What the last computation left on the device, for the entry points that read it back.  An entry point replaces the
// record where it starts enqueueing (after every check), so a refused call leaves the previous result readable.
struct Resident {
    Plan *plan = nullptr;
    int frames = 0, cn = 3, depth = kDepth8U;   // frames, channels and image depth of the pyramid
    bool features = false, resp = false, dp = false;   // the stages held, all for `plan`
    bool c31_zero = false;           // the features were written by the HOG kernels (channel 31 = 0), not uploaded by the caller
    bool latent = false;             // pbd_detect_latent: the result lives in the handle's latent twin (pbd_examples* read it there)
    bool marginals = false;          // pbd_max_marginals: the planes of frame mm_frame are held for this result (whoever replaces
    int mm_frame = 0;                // the record drops them with it)
    void drop_conv() { resp = dp = marginals = false; }   // the filter bank changed (the caller cuts the latent twin's record too)
    void clear() { *this = Resident{}; }
};

// What fail / HIPCHK / guarded / entry work on: where a failure's message goes and the device the object's calls run on.
// The base of pbd_handle and pbd_qp.
struct ErrCtx {
    std::string err;
    int device = 0;
};

extern thread_local std::string g_create_error;   // pbd_last_error(NULL) / pbd_qp_last_error(NULL)

// The members of a handle; pbd_handle itself (the C API's name, global namespace) adds nothing.
struct Handle : ErrCtx {
    pbd_config cfg{};                // as given to pbd_create; the device is read from ErrCtx::device alone
    Stream stream;                   // every kernel of the handle

    // model (host copies)
    int NC = 0, F = 0, flen = 32, sbin = 4, interval = 10, norient = 18, NS = 0, NM = 0, max_parts = 0;
    float thresh = 0.f;
    int ksize = 0, Fpad = 0;
    std::vector<int> filter_ksize, part_offset, parentid, mix_offset, filterid, biasid, defid, ptr_slot, anchors;
    std::vector<float> biasw, defw;
    std::vector<Group> groups;       // deepest first
    std::vector<RootJob> rjobs;
    std::vector<PartWalk> walk;
    std::vector<int> walk_off;
    int JGmax = 0;
    int max_mix = 1;                 // largest number of mixtures of any part
    bool filters_set = false;
    bool seq_mode = false;           // a filter id occurs twice inside a component: sequential schedule, accumulators keyed by filter id
    bool bank_matches_model = true;  // false after a setFilters() whose bank no longer covers the model's filter ids

    // device model tables
    // convolution bank: the filters grouped by size (one class in every known model; the reference builds one engine
    // per filter and so takes any mix: src/SpatialConvolutionEngine.cpp:141-158)
    struct ConvClass {
        int K = 0, nf = 0, Fpad = 0;
        DevBuf wts;                  // real-typed weights of the class
        DevTable<int> fmap;          // class-local index -> filter id (empty when the class is the whole bank in order)
        // k_conv3 (float, 5 x 5): the class cut into units of 2..8 filters, weights [unit][32][25][8]
        DevBuf wts3;
        DevTable<int> unit_f0, unit_ql, unit_woff;
        int nunits = 0;
        DevTable<float> c31tab;      // [81][c31stride]: see pbd_kernels_conv.hip (channel 31)
        int c31stride = 0;
        DevBuf wfrag64;              // PBD_CONV_MFMA_F64: the class's A-fragments (pbd_layout.h, f64_frag_source)
        DevBuf wfrag16;              // PBD_CONV_MFMA_ANY / _F16_ANY: the class's 16-bit A-fragments (any_frag_source); empty for
                                     // an all-5x5 bank, which keeps the records of modes 2 / 3 (d_wrec)
    };
    std::vector<ConvClass> conv_classes;
    DevBuf d_wrec;                   // bf16 hi/lo weight records of the matrix-core path
    DevTable<float> d_biasw;
    DevTable<int> d_walk_off;
    DevTable<RootJob> d_rjobs;
    DevTable<PartWalk> d_walk;
    DevBuf d_coord;                  // HogCoordT<R>[]
    int coord_n = 0;
    DevBuf d_coord_fine;             // the same table for the fine octave's bin size sbin / 2 (built while fine_octave is on)
    int coord_fine_n = 0;
    bool f64 = false;                // reference template parameter T = double
    size_t rs = sizeof(float);       // sizeof(T)
    bool resp_half = false;          // conv_is_f16(mode): the responses live on the device as fp16 (BASELINE configs[4])
    size_t resp_es = sizeof(float);  // bytes per response element on the device

    // plans
    std::vector<std::unique_ptr<Plan>> plans;
    Resident res;
    int shard_rank = 0, shard_world = 1;   // level sharding of single frames over several GPUs (pbd_set_level_shard)
    bool fine_octave = false;        // pbd_set_fine_octave: every image plan built afterwards carries the octave; the latent twin follows
    int padx = 0, pady = 0;          // the padded pyramid (pbd_set_padding): every plan built afterwards carries it; the latent twin follows
    int walk_mode = 0;               // PBD_WALK_* (pbd_set_walk), read when a walk is enqueued; the latent twin follows its handle
    bool nms = false;                // per-frame sort + non-maxima suppression of the list (pbd_set_nms), latched at enqueue
    float nms_overlap = 0.f;
    int root_nms = 0;                // grid NMS of the root scores before the find (pbd_set_root_nms): window size, 0 = off; read at enqueue
    int top_k = 0;                   // the K best roots of each frame before the find (pbd_set_top_k): 0 = off; read at enqueue
    int scale_nms = -1;              // scale NMS of the roots before top-K and the find (pbd_set_scale_nms): dl, -1 = off; read at enqueue
    int gn_lanes = 0;                // forced lanes per block of k_grid_nms, 1 or 64; 0: by sz (pbd_debug_set_option)
    // scale-depth pruning of the roots before the find (pbd_set_depth_prune; read at enqueue) and the depth images bound to the
    // next detect call (pbd_bind_depth*): their frame table, the host form's copies, the byte per root cell.  claim_depth moves
    // a binding that fits the call into `dpr_call` (on the device: dpr_tab); enqueue_argmin uses it once
    bool dprune = false;
    DepthPruneRule dprune_rule{};
    struct DepthBind { std::vector<Box3dFrame> tab; int depth = 0; } dpr_bound, dpr_call;
    StagedTable dpr_tab;
    DevBuf dpr_depth, dpr_ok;
    // pbd_depth_prune*: the frame table, the workspace (flags and block counts); the host form shares pbd_depth_consistency's
    // image, record and output buffers
    StagedTable dpl_tab;
    DevBuf dpl_ws;
    DtOptions dt_opt;               // forced distance-transform launch choices (pbd_debug_set_option)
    int dp_budget_mb = 0;            // DP scratch budget per chunk of frames; 0: 8 GB (pbd_debug_set_option)
    bool hog_two_pass = false;       // the histogram stage never takes the fused kernel (pbd_debug_set_option)

    // workspace
    DevBuf frames, pyr, gmag, gori, hist, norm, feat, resp, acc, Ik, rootv, rooti;
    int totmix = 0;                  // (part, mixture) pairs of the model = planes of IxRaw / IyRaw per cell block
    DevBuf tmp, dt, IxRaw, IyRaw, stk, scales_tmp, find_blk;
    DevBuf post_ws;                  // workspace of the post-processing stage (pbd_kernels_post.hip)
    // grid NMS: the detect path's byte per root cell (pbd_set_root_nms); pbd_grid_nms*: the plane table (staged as the tables
    // below), the host form's planes, masks and bytes
    DevBuf gn_max;
    StagedTable gn_tab;
    DevBuf gn_src, gn_mask, gn_dst;
    // top-K: the detect path's byte per root cell (pbd_set_top_k) and the selection's workspace (histograms, segment states, tile
    // counts); pbd_top_k_cells*: the segment table (staged as the tables below), the host form's values, masks and bytes;
    // pbd_top_k*: the workspace (flags and block counts), the host form's records and output
    DevBuf tk_keep, tk_ws;
    StagedTable tk_tab;
    DevBuf tk_src, tk_mask, tk_dst;
    DevBuf tkl_ws, tkl_in, tkl_out;
    // scale NMS: the detect path's byte per root cell (pbd_set_scale_nms); pbd_scale_nms*: the workspace (flags and block counts),
    // the host form's records and output
    DevBuf sn_keep;
    DevBuf snl_ws, snl_in, snl_out;
    DevBuf dbg_in, dbg_out;          // pbd_debug_postprocess
    // pbd_boxes3d*: the frame table (staged in pinned memory, rewritten only once its previous copy has completed); the host
    // form's depth images, records and boxes.  Never the detect path's buffers: the resident result stays readable.
    StagedTable b3_tab;
    DevBuf b3_depth, b3_rec, b3_out;
    // pbd_boxes3d_camera*: the pinhole table (staged as the frame table), k_boxes3d's cubes, the host form's outputs
    StagedTable cam_tab;
    DevBuf cam_cube, cam_out;
    // pbd_cluster_objects*: the cloud table (staged as above), the workspace, the host form's clouds, payload, boxes and outputs
    StagedTable cl_tab;
    DevBuf cl_ws, cl_cloud, cl_in, cl_out;
    long long cl_crop_cap = 0;       // the host form's crop capacity so far (grows to what a call needed)
    // pbd_remove_planes*: the cloud table (staged as above), the workspace, the host form's packed clouds and outputs
    StagedTable pl_tab;
    DevBuf pl_ws, pl_cloud, pl_out;
    // pbd_depth_consistency*: the frame table (staged as above), the model's edge tables (built on first use), the workspace,
    // the host form's depth images, records and output
    StagedTable dc_tab;
    DevBuf dc_ws, dc_depth, dc_rec, dc_out;
    DevTable<int> dc_part_offset, dc_parent;
    DevTable<double> dc_norm;
    // pbd_suppress*: the canvas plan of the last list of frame sizes, the check flag, the host form's records and output
    std::unique_ptr<Plan> sup_plan;
    DevBuf sup_bad, sup_in, sup_out;
    // pbd_candidate_mask*: the frame table (staged as above), the workspace (hulls, frame ranges, the bad flag), the host form's
    // records, frames and labels, and its status word
    StagedTable mk_tab;
    DevBuf mk_ws, mk_rec, mk_img;
    // pbd_part_poses: the host form's inputs and outputs
    DevBuf ps_buf;
    // pbd_part_nms* / pbd_best_overlap* / pbd_eval_pck* / pbd_eval_apk*: the ground truth of a call (staged as the frame
    // tables), the workspace, the host forms' inputs and outputs
    StagedTable ev_tab;
    DevBuf ev_ws, ev_in, ev_out;
    // pbd_model_vector / pbd_examples*: the model vector in T (built by build_model), the filter sizes and offsets of the model the
    // handle was created with, the strides of an example, the walk's tables (uploaded on first use), the (record, part) workspace,
    // the host form's records and outputs
    std::vector<char> mvec;
    std::vector<int> model_ksize;
    std::vector<long long> model_foff;   // offset of filter f in the model vector
    int nbias = 0, ndefs = 0, ex_hdr_words = 0, ex_values = 0;
    DevTable<ExGm> ex_gm;
    DevTable<int> ex_anchors;
    DevTable<long long> ex_foff;
    DevBuf ex_ws, ex_rec, ex_out;
    // pbd_part_scores* / pbd_score_placements*: the model's tables (per (part, mixture) ids with this handle's filter ids,
    // anchors, mixtures per part; uploaded on first use), the call's deformation weights (staged: a model update changes them),
    // the placements when the caller takes none, the host form's records, placements and outputs
    DevTable<ExGm> sc_gm;
    DevTable<int> sc_anchors, sc_nmix;
    StagedTable sc_defw;
    DevBuf sc_ws, sc_rec, sc_out;
    // pbd_max_marginals / pbd_marginal_poses*: the planes of one frame (values, down, parent pointers, messages), the scratch
    // of a slice of mirrored transforms (context planes and the transforms' pointer planes; their values and envelope stacks are
    // the dynamic program's own scratch), the call's job tables (one staged block), the model's types per part (uploaded on first
    // use), the decode's scales, the host form's seeds and outputs
    DevBuf mm_val, mm_down, mm_jx, mm_jy, mm_jk, mm_msg, mm_ctx, mm_six, mm_siy;
    StagedTable mm_tab;
    DevTable<int> mm_nmix;
    DevBuf mm_scales, mm_in, mm_out, mm_place;
    // pbd_set_model_vector* / pbd_qp_apply: the model vector on the device (T; written by the first update, from then on the
    // source of every weight table), whether the host copy `mvec` is behind it (brought up to date on demand: sync_mvec), the
    // update's index tables (built on first use), the host form's vector, and the status block {refused, -, -, -, biasw, defw}
    // with its pinned mirror
    DevBuf d_mvec;
    bool mvec_stale = false;
    bool broken = false;             // a model update failed after its kernels were queued: check_bank refuses the handle
    DevTable<int> mu_gm_def, mu_root_bias;
    DevTable<MuJobRef> mu_jobs;
    DevTable<long long> mu_foff;
    DevBuf mu_src, mu_status;
    HostBuf mu_status_host;
    // pbd_detect_latent: a second handle on the same stream whose model gives every (component, part, mixture) its own filter
    // (the mask belongs to the (component, part, mixture), not to a shared filter), created on first use; the part -> mixture
    // table of its bank, the call's boxes / mixtures and its payload.  The detect path of this handle never touches it.
    std::unique_ptr<pbd_handle, void (*)(pbd_handle *)> lat{nullptr, pbd_destroy};
    DevTable<int4> lat_gm;
    DevBuf lat_in, lat_pay;
    // pbd_cluster_parts*: the call's tables (parts and starting points in one staged block), the per-pair workspace, the host
    // form's offsets and outputs
    StagedTable km_tab;
    DevBuf km_ws, km_in, km_out;
    // mixed-size calls: the FrameDesc table
    StagedTable fd_tab;
    // pbd_warp_positives*: the plan whose levels are the kept boxes' patches (rebuilt when the kept count or the patch size
    // changes), the call's tables (frames, boxes, taps and coefficients in one staged block), the host form's outputs
    std::unique_ptr<Plan> wp_plan;
    StagedTable wp_tab;
    DevBuf wp_out;
    // pbd_augment_frames*: the call's job and tile tables (one staged block); the host form's packed sources and destinations.
    // Buffers of their own: the call leaves the detect path's buffers and the resident result alone
    StagedTable aug_tab;
    DevBuf aug_buf;

    // A candidate list on its way out.  The device side is the "payload" the find / walk kernels write: word 0 = roots
    // found, then the records, already in (frame, level, component, y, x) order.  The host side is a pinned mirror: the
    // count and the first `guess` records (what the previous batch needed + 25 %) are copied by ONE asynchronous D2H
    // enqueued right behind the walk kernel, so a steady stream of batches never waits for a count before it can ask for
    // the records; a batch that outgrows the guess costs one more copy.
    struct CandBuf {
        DevBuf payload;
        DevBuf post;                                      // the suppressed list when `nms` (then the read-back source)
        bool nms = false;                                 // the stage was on when this list was enqueued
        HostBuf host;
        int copied = 0;                                   // records covered by the enqueued copy
        const DevBuf &out() const { return nms ? post : payload; }
        int32_t *words() const { return host.as<int32_t>(); }
        hipError_t reserve(size_t words) { return host.ensure(words * 4, (words + words / 4 + 256) * 4); }
    } cb;
    int cand_guess = 1024;                                // records the next speculative copy covers (shared by every CandBuf)

    // pipelined host entry points (pbd_detect_batch_submit / _wait): two batches may be in flight
    struct Slot {
        HostBuf pinned;                                   // host staging of the frames
        DevBuf frames;
        CandBuf cb;
        Event copied, done;
    } slot[2];
    Stream stream_copy, stream_d2h;
    long long nsubmitted = 0, nwaited = 0;

    Prof prof;
};

}  // namespace pbd

struct pbd_handle : pbd::Handle {};

namespace pbd {

// stores the message in h->err (no object yet: in g_create_error) and returns `code`
int fail(ErrCtx *h, int code, const char *fmt, ...);

#define HIPCHK(h, expr)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (void)hipGetLastError();   /* the error is reported through the status code, not left sticky */ \
            return fail(h, e_ == hipErrorOutOfMemory ? PBD_ERR_NOMEM : PBD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                 \
        }                                                                                           \
    } while (0)

// "No exception crosses this ABI" (include/pbd.h): every extern "C" body runs inside guarded().  The
// reference's errors on this path are CV_Error / bool returns, never process death
// (src/HOGFeatures.cpp:141-145, src/FileStorageModel.cpp:100-101).
template <class F>
int guarded(ErrCtx *h, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(h, PBD_ERR_NOMEM, "out of host memory");
    } catch (const std::length_error &e) {
        return fail(h, PBD_ERR_NOMEM, "host allocation too large: %s", e.what());
    } catch (const std::exception &e) {
        return fail(h, PBD_ERR_INVALID, "unexpected exception: %s", e.what());
    } catch (...) {
        return fail(h, PBD_ERR_INVALID, "unexpected exception");
    }
}

// The preamble of every entry point that takes a handle or a QP: a null object or pointer argument (`args_ok` false) is
// PBD_ERR_INVALID, then the object's device is made current and, for a handle with kIdle, a call while a batch is in flight is
// refused.  The body then checks argument values and the object's state before it enqueues or copies anything.
template <class F>
int entry(ErrCtx *h, bool args_ok, F &&body) noexcept
{
    return guarded(h, [&]() -> int {
        if (!h || !args_ok) return PBD_ERR_INVALID;
        (void)hipSetDevice(h->device);
        return body();
    });
}
enum InFlight { kBusyOk, kIdle };
template <class F>
int entry(pbd_handle *h, bool args_ok, InFlight need, F &&body) noexcept
{
    return entry(static_cast<ErrCtx *>(h), args_ok, [&]() -> int {
        if (need == kIdle && h->nsubmitted != h->nwaited) return fail(h, PBD_ERR_STATE, "a submitted batch has not been waited for");
        return body();
    });
}

inline int StagedTable::stage(pbd_handle *h, const void *src, size_t bytes)
{
    if (copied.p) HIPCHK(h, hipEventSynchronize(copied.p));   // the previous call's table has left the staging buffer
    else HIPCHK(h, hipEventCreateWithFlags(&copied.p, hipEventDisableTiming));
    HIPCHK(h, host.ensure(bytes, bytes * 2 + 256));
    HIPCHK(h, dev.ensure(bytes));
    memcpy(host.p, src, bytes);
    HIPCHK(h, hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(copied.p, h->stream));
    return PBD_OK;
}

// Both passes of `pieces(Carve &)` over `buf`: the sizing pass, `buf` grown to its total (`exact`: allocated anew at exactly
// that), the carving pass.  A carving pass that ends anywhere else than the sizing pass did is refused.
template <class F>
int carve(ErrCtx *h, DevBuf &buf, F &&pieces, bool exact = false)
{
    Carve size;
    pieces(size);
    HIPCHK(h, exact ? buf.alloc_exact(size.off) : buf.ensure(size.off));
    Carve c{buf.as<uint8_t>()};
    pieces(c);
    if (c.off != size.off || c.pieces != size.pieces || c.off > buf.size)
        return fail(h, PBD_ERR_STATE, "workspace layout: carved %zu bytes of %zu planned, %zu held", c.off, size.off, buf.size);
    return PBD_OK;
}

// shared checks (also check_frames below): PBD_OK (0) or the failure's status code
inline int check_batch(pbd_handle *h, int nframes)
{
    if (nframes >= 1 && nframes <= h->cfg.max_batch) return PBD_OK;
    return fail(h, PBD_ERR_INVALID, "nframes %d outside 1..max_batch %d", nframes, h->cfg.max_batch);
}
inline int check_bank(pbd_handle *h)
{
    if (h->broken) return fail(h, PBD_ERR_STATE, "an earlier model update failed half way: the handle must be destroyed");
    if (h->bank_matches_model) return PBD_OK;
    return fail(h, PBD_ERR_STATE, "the filter bank set by setFilters() (%d filters) does not cover the model's filter ids", h->F);
}

inline int stride(const pbd_handle *h) { return 8 + 4 * h->max_parts; }   // int32 words per candidate record

// While a ProfScope is alive, every kernel launched by this thread is timed under kernel id `k` (see PBD_LAUNCH).
struct ProfScope {
    pbd_handle *h; int k; ProfHook hook; ProfHook *prev;
    static void take(void *ctx, hipEvent_t *a, hipEvent_t *b)
    {
        ProfScope *self = static_cast<ProfScope *>(ctx);
        Prof &prof = self->h->prof;
        Prof::Rec r{self->k, prof.get(), prof.get()};
        *a = r.a.p; *b = r.b.p;
        prof.recs.push_back(std::move(r));
    }
    ProfScope(pbd_handle *h_, int k_, hipStream_t) : h(h_), k(k_), hook{this, &ProfScope::take}, prev(g_prof_hook)
    {
        if (h->prof.on == 1 || (h->prof.on == 2 && k == PBD_K_CONV)) g_prof_hook = &hook;
    }
    ~ProfScope() { g_prof_hook = prev; }
    ProfScope(const ProfScope &) = delete;
    ProfScope &operator=(const ProfScope &) = delete;
};

// a (frame, level) of the resident result -> (frame index into the buffers, level of the plan); mixed plans: frame 0, the
// frame's level in the virtual table
inline bool resident_level(const Resident &r, int frame, int level, int *bf, int *bl)
{
    const Plan &P = *r.plan;
    if (P.kind == 2) {
        if (frame < 0 || frame >= P.mixed_frames || level < 0 || level >= P.frame_lv0[frame + 1] - P.frame_lv0[frame]) return false;
        *bf = 0; *bl = P.frame_lv0[frame] + level;
        return true;
    }
    if (frame < 0 || frame >= r.frames || level < 0 || level >= P.nlevels) return false;
    *bf = frame; *bl = level;
    return true;
}

// the handle whose buffers hold the resident result: the latent twin after pbd_detect_latent (pbd_examples*, pbd_get_stage)
inline pbd_handle *resident_owner(pbd_handle *h) { return h->res.latent && h->lat ? h->lat.get() : h; }

// ---- defined in pbd_capi.hip, called from the other files of the entry layer (see the definitions)
void post_canvas_plan(Plan &M);
// what restricts the roots a find lists beyond the threshold: the window of pbd_set_root_nms (0: off) and whether the depth images
// claimed for the call (h->dpr_call) prune them (pbd_set_depth_prune).  The detect entry points pass root_sel(h); DynamicProgram::
// argmin, the latent search and the trainers' re-walks pass none
struct RootSel { int nms = 0; bool prune = false; int top = 0; int scale = -1; };   // top: the K of pbd_set_top_k (0: off); scale: the dl of pbd_set_scale_nms (-1: off)
inline RootSel root_sel(const pbd_handle *h) { return {h->root_nms, !h->dpr_call.tab.empty(), h->top_k, h->scale_nms}; }
int enqueue_argmin(pbd_handle *h, Plan &P, int nframes, const float *d_scales, int frame_offset, int32_t *d_payload, int capacity,
                   hipStream_t st, bool walk_only = false, RootSel sel = {});
int enqueue_post(pbd_handle *h, int nframes, int rows, int cols, float overlap, const int32_t *d_in, int in_cap, int frame_offset,
                 int32_t *d_out, int out_cap, hipStream_t st, const Plan *mixed = nullptr, int in_offset = 0, int *bad = nullptr);
int depth_prune_rule(pbd_handle *h, const pbd_depth_prune_cfg &cfg, DepthPruneRule *rule);
// the selection's workspace carved from h->tk_ws for p.nseg segments and p.ntiles tiles, its histograms zeroed on `st`
int top_k_workspace(pbd_handle *h, TopKParams &p, hipStream_t st);
int check_frames_mixed(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host, Plan **plan);
int enqueue_detect_mixed(pbd_handle *h, Plan &P, int nframes, const pbd_frame *frames, int cn, int depth, bool host,
                         const LatentParams *mask = nullptr);
// the depth, channel and per-frame checks of a mixed-size call (no plan is made); the frames' descriptors on the device side:
// host frames are packed into the handle's frame buffer (copies enqueued on its stream), device frames are read in place
int check_frame_descs(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host);
int frame_descs(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host, std::vector<FrameDesc> &fd);
// pbd_warp_positives*: the plan of n patches of P x P pixels (h->wp_plan) with the pyramid and HOG workspaces sized for it;
// the HOG stage over the patches k_warp wrote into h->pyr
int warp_plan(pbd_handle *h, int n, int P, int cn, int depth, Plan **out);
void warp_hog(pbd_handle *h, Plan &W, int cn, int depth);

}  // namespace pbd

#pragma GCC visibility pop
