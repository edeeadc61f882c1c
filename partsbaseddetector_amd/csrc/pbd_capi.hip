// pbd_capi.hip -- handle, plans, device workspace and the C entry points of include/pbd.h.
//
// Host logic restated from the reference for this path:
//   pyramid geometry            src/HOGFeatures.cpp:95-127, include/HOGFeatures.hpp:74-81
//   engine wiring               src/PartsBasedDetector.cpp:69-127
//   Parts index tables          include/Parts.hpp:172-187
// There is no CPU compute path: every stage runs as a HIP kernel (pbd_kernels_*.hip).
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

using namespace pbd;

namespace pbd {
thread_local ProfHook *g_prof_hook = nullptr;
}

namespace {

thread_local std::string g_create_error;

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

// ---- pyramid geometry (host) -------------------------------------------------------------------
// Overload resolution assumed for the reference's expressions: C++11 <cmath>, i.e. pow(float,float)
// and log(float) are the float versions, pow(float,int) promotes to double.
int plan_pyramid(int rows, int cols, int sbin, int interval, std::vector<int> &lr, std::vector<int> &lc,
                 std::vector<float> &scales)
{
    const float sfactor = powf(2.0f, 1.0f / (float)interval);             // HOGFeatures.hpp:78
    const float h = (float)rows, w = (float)cols;
    const float mn = std::min(h, w);
    const float ns = 1 + floorf(logf(mn / (5.0f * (float)sbin)) / logf(sfactor));   // HOGFeatures.cpp:99
    if (!(ns >= 1)) return 0;
    const int n = (int)ns;
    if (n > PBD_MAX_LEVELS) return -1;
    if (n < interval) return -2;   // the reference writes out of bounds here (HOGFeatures.cpp:114-118)
    lr.assign(n, 0); lc.assign(n, 0); scales.assign(n, 0.f);
    for (int i = 0; i < interval; ++i) {
        const float f = (float)((double)1.0f / pow((double)sfactor, (double)i));     // :116
        lc[i] = (int)lrint((double)(w * f));   // Size_<float> -> Size: cvRound, half to even
        lr[i] = (int)lrint((double)(h * f));
        scales[i] = (float)(pow((double)sfactor, (double)i) * (double)sbin);          // :118
        for (int j = i + interval; j < n; j += interval) {                            // :120-126
            lc[j] = (lc[j - interval] + 1) / 2;
            lr[j] = (lr[j - interval] + 1) / 2;
            scales[j] = 2 * scales[j - interval];
        }
    }
    return n;
}

inline short sat_short_round(float v)
{
    long iv = lrint((double)v);
    return (short)(iv < -32768 ? -32768 : iv > 32767 ? 32767 : iv);
}

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
    int ntiles = 0;
    // device tables
    DevTable<LevelDesc> d_lv;
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
    // dynamic program in groups of whole frames when the virtual frame's scratch exceeds the budget: sub-plans whose cell
    // offsets start at 0 (cell0 = the group's first cell in the virtual frame), built for `chunk_budget`
    size_t chunk_budget = 0;
    std::vector<std::unique_ptr<Plan>> chunk_plans;
    std::vector<long long> chunk_cell0;
};

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
    void drop_conv() { resp = dp = false; }   // the filter bank changed
    void clear() { *this = Resident{}; }
};

}  // namespace

struct pbd_handle {
    pbd_config cfg{};
    std::string err;
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
        DevBuf wfrag64;              // PBD_CONV_MFMA_F64: the class's A-fragments (pbd_internal.h, f64_passes)
    };
    std::vector<ConvClass> conv_classes;
    DevBuf d_wrec;                   // bf16 hi/lo weight records of the matrix-core path
    DevTable<float> d_biasw;
    DevTable<int> d_walk_off;
    DevTable<RootJob> d_rjobs;
    DevTable<PartWalk> d_walk;
    DevBuf d_coord;                  // HogCoordT<R>[]
    int coord_n = 0;
    bool f64 = false;                // reference template parameter T = double
    size_t rs = sizeof(float);       // sizeof(T)
    bool resp_half = false;          // PBD_CONV_MFMA_F16: the responses live on the device as fp16 (BASELINE configs[4])
    size_t resp_es = sizeof(float);  // bytes per response element on the device

    // plans
    std::vector<std::unique_ptr<Plan>> plans;
    Resident res;
    int shard_rank = 0, shard_world = 1;   // level sharding of single frames over several GPUs (pbd_set_level_shard)
    bool nms = false;                // per-frame sort + non-maxima suppression of the list (pbd_set_nms), latched at enqueue
    float nms_overlap = 0.f;
    DtOptions dt_opt;                // forced distance-transform launch choices (pbd_debug_set_option)
    int dp_budget_mb = 0;            // DP scratch budget per chunk of frames; 0: 8 GB (pbd_debug_set_option)

    // workspace
    DevBuf frames, pyr, gmag, gori, hist, norm, feat, resp, acc, Ik, rootv, rooti;
    int totmix = 0;                  // (part, mixture) pairs of the model = planes of IxRaw / IyRaw per cell block
    DevBuf tmp, dt, IxRaw, IyRaw, stk, scales_tmp, find_blk;
    DevBuf post_ws;                  // workspace of the post-processing stage (pbd_kernels_post.hip)
    DevBuf dbg_in, dbg_out;          // pbd_debug_postprocess
    // pbd_boxes3d*: the frame table (staged in pinned memory, rewritten only once its previous copy has completed); the host
    // form's depth images, records and boxes.  Never the detect path's buffers: the resident result stays readable.
    HostBuf b3_tab_host;
    DevBuf b3_tab, b3_depth, b3_rec, b3_out;
    Event b3_tab_copied;
    // pbd_boxes3d_camera*: the pinhole table (staged as the frame table), k_boxes3d's cubes, the host form's outputs
    HostBuf cam_tab_host;
    DevBuf cam_tab, cam_cube, cam_out;
    Event cam_tab_copied;
    // pbd_cluster_objects*: the cloud table (staged as above), the workspace, the host form's clouds, payload, boxes and outputs
    HostBuf cl_tab_host;
    DevBuf cl_tab, cl_ws, cl_cloud, cl_in, cl_out;
    Event cl_tab_copied;
    long long cl_crop_cap = 0;       // the host form's crop capacity so far (grows to what a call needed)
    // pbd_remove_planes*: the cloud table (staged as above), the workspace, the host form's packed clouds and outputs
    HostBuf pl_tab_host;
    DevBuf pl_tab, pl_ws, pl_cloud, pl_out;
    Event pl_tab_copied;
    // pbd_depth_consistency*: the frame table (staged as above), the model's edge tables (built on first use), the workspace,
    // the host form's depth images, records and output
    HostBuf dc_tab_host;
    DevBuf dc_tab, dc_ws, dc_depth, dc_rec, dc_out;
    Event dc_tab_copied;
    DevTable<int> dc_part_offset, dc_parent;
    DevTable<double> dc_norm;
    // pbd_suppress*: the canvas plan of the last list of frame sizes, the check flag, the host form's records and output
    std::unique_ptr<Plan> sup_plan;
    DevBuf sup_bad, sup_in, sup_out;
    // pbd_candidate_mask*: the frame table (staged as above), the workspace (hulls, frame ranges, the bad flag), the host form's
    // records, frames and labels, and its status word
    HostBuf mk_tab_host;
    DevBuf mk_tab, mk_ws, mk_rec, mk_img;
    Event mk_tab_copied;
    // pbd_part_poses: the host form's inputs and outputs
    DevBuf ps_buf;
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
    // pbd_detect_latent: a second handle on the same stream whose model gives every (component, part, mixture) its own filter
    // (the mask belongs to the (component, part, mixture), not to a shared filter), created on first use; the part -> mixture
    // table of its bank, the call's boxes / mixtures and its payload.  The detect path of this handle never touches it.
    std::unique_ptr<pbd_handle, void (*)(pbd_handle *)> lat{nullptr, pbd_destroy};
    DevTable<int4> lat_gm;
    DevBuf lat_in, lat_pay;
    // mixed-size calls: the FrameDesc table, staged in pinned memory (rewritten only once its previous copy has completed)
    HostBuf fd_host;
    DevBuf fd_dev;
    Event fd_copied;

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

namespace {

int fail(pbd_handle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try {
        if (h) h->err = buf; else g_create_error = buf;
    } catch (...) {   // the message itself could not be stored: the status code still goes out
    }
    return code;
}

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
int guarded(pbd_handle *h, F &&body) noexcept
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

// The preamble of every entry point that takes a handle: a null handle or pointer argument (`args_ok` false) is
// PBD_ERR_INVALID, then the handle's device is made current and, with kIdle, a call while a batch is in flight is refused.
// The body then checks argument values and handle state before it enqueues or copies anything.
enum InFlight { kBusyOk, kIdle };
template <class F>
int entry(pbd_handle *h, bool args_ok, InFlight need, F &&body) noexcept
{
    return guarded(h, [&]() -> int {
        if (!h || !args_ok) return PBD_ERR_INVALID;
        (void)hipSetDevice(h->cfg.device);
        if (need == kIdle && h->nsubmitted != h->nwaited) return fail(h, PBD_ERR_STATE, "a submitted batch has not been waited for");
        return body();
    });
}

// shared checks (also check_frames below): PBD_OK (0) or the failure's status code
int check_batch(pbd_handle *h, int nframes)
{
    if (nframes >= 1 && nframes <= h->cfg.max_batch) return PBD_OK;
    return fail(h, PBD_ERR_INVALID, "nframes %d outside 1..max_batch %d", nframes, h->cfg.max_batch);
}
int check_bank(pbd_handle *h)
{
    if (h->bank_matches_model) return PBD_OK;
    return fail(h, PBD_ERR_STATE, "the filter bank set by setFilters() (%d filters) does not cover the model's filter ids", h->F);
}

int stride(const pbd_handle *h) { return 8 + 4 * h->max_parts; }   // int32 words per candidate record

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

// ---- plan construction -------------------------------------------------------------------------
// Cover a rows x cols level with 256-cell tiles of shape 32x8, 16x16 or 8x32 (shape k: 32>>k wide, 8<<k
// high) so that the fewest lanes compute cells outside the level: a dynamic program over the columns picks
// the vertical strips, each strip is then cut into tiles of its shape.
static void cover_level(int l, int rows, int cols, std::vector<ConvTile> *shaped)
{
    const long long INF = 1LL << 60;
    std::vector<long long> cost(cols + 1, INF);
    std::vector<int> pick(cols + 1, -1);
    cost[0] = 0;
    for (int w = 1; w <= cols; ++w)
        for (int k = 0; k < 3; ++k) {
            const int tw = kConvTW >> k, th = kConvTH << k;
            const int prev = std::max(w - tw, 0);
            const long long c = cost[prev] + (long long)tw * ((rows + th - 1) / th) * th;
            if (c < cost[w]) { cost[w] = c; pick[w] = k; }
        }
    std::vector<std::pair<int, int>> strips;   // (x0, shape), right to left
    for (int w = cols; w > 0;) {
        const int k = pick[w], tw = kConvTW >> k;
        const int x0 = std::max(w - tw, 0);
        strips.push_back({x0, k});
        w = x0;
    }
    for (auto it = strips.rbegin(); it != strips.rend(); ++it) {
        const int k = it->second, th = kConvTH << k;
        for (int y0 = 0; y0 < rows; y0 += th) shaped[k].push_back({l, y0, it->first});
    }
}

// Tiles of the exact 5 x 5 convolution for a launch of `nb` frames (pbd_kernels_conv.hip): the strips of four rows of every
// level of every frame, left to right, form one sequence of positions; a tile takes 64 consecutive positions, in at most
// kConvMaxSeg runs (a run stays inside one strip) -- when a fourth run would be needed the tile ends early.
void build_seg_tiles(const std::vector<LevelDesc> &lv, int nb, std::vector<ConvSegTile> &out)
{
    out.clear();
    ConvSegTile cur{};
    int lanes = 0;
    auto flush = [&]() { if (cur.nseg) out.push_back(cur); cur = ConvSegTile{}; lanes = 0; };
    for (int f = 0; f < nb; ++f)
        for (int l = 0; l < (int)lv.size(); ++l) {
            const int H = lv[l].rows, W = lv[l].cols;
            if (H <= 0 || W <= 0) continue;
            for (int st = 0; st < (H + 3) / 4; ++st)
                for (int x = 0; x < W;) {
                    if (cur.nseg == kConvMaxSeg || lanes == 64) flush();
                    const int take = std::min(W - x, 64 - lanes);
                    cur.len[cur.nseg] = take;
                    cur.seg[cur.nseg] = ConvSeg{f, l, st, x};
                    cur.nseg += 1;
                    lanes += take;
                    x += take;
                }
        }
    flush();
}

hipError_t finish_plan_tables(Plan &P, int sbin)
{
    // flat row / column lookup and conv tiles over the feature maps
    std::vector<int> row2level, rowoff(P.nlevels + 1, 0), col2level, coloff(P.nlevels + 1, 0);
    std::vector<ConvTile> tiles, shaped[3], htiles;
    P.quad_per_frame = 0;
    for (int l = 0; l < P.nlevels; ++l) {
        P.lv[l].quad_off = P.quad_per_frame;
        P.quad_per_frame += ((long long)P.lv[l].rows * P.lv[l].cols + 3) / 4;
        const LevelDesc &d = P.lv[l];
        for (int by0 = 0; by0 < d.blk_rows && d.blk_cols > 0; by0 += hog_tile_rows(sbin))
            for (int bx0 = 0; bx0 < d.blk_cols; bx0 += kHogTBX) htiles.push_back({l, by0, bx0});
        rowoff[l] = (int)row2level.size();
        coloff[l] = (int)col2level.size();
        if (d.rows > 0 && d.cols > 0) {
            for (int y = 0; y < d.rows; ++y) row2level.push_back(l);
            for (int x = 0; x < d.cols; ++x) col2level.push_back(l);
            for (int y0 = 0; y0 < d.rows; y0 += kConvTH)
                for (int x0 = 0; x0 < d.cols; x0 += kConvTW) tiles.push_back({l, y0, x0});
            cover_level(l, d.rows, d.cols, shaped);
        }
    }
    {
        int longest = 0;
        for (const LevelDesc &d : P.lv) longest = std::max(longest, std::max(d.rows, d.cols));
        P.ptr8 = longest <= 256;
        P.longest = longest;
    }
    rowoff[P.nlevels] = (int)row2level.size();
    coloff[P.nlevels] = (int)col2level.size();
    P.nrows_flat = (int)row2level.size();
    P.ncols_flat = (int)col2level.size();
    P.ntiles = (int)tiles.size();
    P.nhtiles = (int)htiles.size();
    // wave-private stack regions: a wave of 64 flat rows (columns) needs 64 x ceil(longest row in the wave / 2)
    // two-entry records; levels are ordered large to small, but take the maximum to be safe
    std::vector<long long> srow, scol;
    long long tot_r = 0, tot_c = 0;
    for (int w0 = 0; w0 < P.nrows_flat; w0 += 64) {
        int mx = 0;
        for (int r = w0; r < std::min(w0 + 64, P.nrows_flat); ++r) mx = std::max(mx, P.lv[row2level[r]].cols);
        srow.push_back(tot_r);
        tot_r += 64LL * ((mx + 1) / 2);
    }
    for (int w0 = 0; w0 < P.ncols_flat; w0 += 64) {
        int mx = 0;
        for (int c = w0; c < std::min(w0 + 64, P.ncols_flat); ++c) mx = std::max(mx, P.lv[col2level[c]].rows);
        scol.push_back(tot_c);
        tot_c += 64LL * ((mx + 1) / 2);
    }
    P.stk_per_jf = std::max(tot_r, tot_c);
    std::vector<ConvTile> all;
    for (int k = 0; k < 3; ++k) { P.nshaped[k] = (int)shaped[k].size(); all.insert(all.end(), shaped[k].begin(), shaped[k].end()); }
    hipError_t e;
    if ((e = P.d_stk_row_off.upload(srow)) != hipSuccess) return e;
    if ((e = P.d_stk_col_off.upload(scol)) != hipSuccess) return e;
    if ((e = P.d_lv.upload(P.lv)) != hipSuccess) return e;
    if ((e = P.d_tiles.upload(tiles)) != hipSuccess) return e;
    if ((e = P.d_shaped.upload(all)) != hipSuccess) return e;
    if ((e = P.d_htiles.upload(htiles)) != hipSuccess) return e;
    if ((e = P.d_row2level.upload(row2level)) != hipSuccess) return e;
    if ((e = P.d_rowoff.upload(rowoff)) != hipSuccess) return e;
    if ((e = P.d_col2level.upload(col2level)) != hipSuccess) return e;
    if ((e = P.d_coloff.upload(coloff)) != hipSuccess) return e;
    return P.d_scales.upload(P.scales);
}

// A finished plan joins the cache; the cache holds at most 16 plans and never evicts the plan the handle's
// resident result refers to.
void cache_plan(pbd_handle *h, std::unique_ptr<Plan> P)
{
    h->plans.push_back(std::move(P));
    while (h->plans.size() > 16) {
        auto it = h->plans.begin();
        if (it->get() == h->res.plan) ++it;
        h->plans.erase(it);
    }
}

// The host side of an image plan (no device work): level table, scales and resize tables of an unsharded rows x cols frame.
// PBD_OK, or PBD_ERR_INVALID with the reason in `err`.
int image_plan_host(int rows, int cols, int sbin, int interval, Plan &Pr, std::string &err)
{
    Plan *P = &Pr;
    char buf[160];
    std::vector<int> lr, lc;
    std::vector<float> scales;
    const int n = plan_pyramid(rows, cols, sbin, interval, lr, lc, scales);
    if (n <= 0) {
        snprintf(buf, sizeof buf, "frame %dx%d too small for sbin %d / interval %d (nscales %d)", rows, cols, sbin, interval, n);
        err = buf;
        return PBD_ERR_INVALID;
    }
    P->kind = 0; P->rows = rows; P->cols = cols;
    P->nlevels = n; P->scales = scales; P->interval = interval;
    P->lv.resize(n);
    std::vector<ResizeTabX> tabx;
    std::vector<ResizeTabY> taby;
    std::vector<ResizeTabXf> tabxf;
    std::vector<ResizeTabYf> tabyf;
    long long pix = 0, blk = 0, cell = 0;
    for (int l = 0; l < n; ++l) {
        LevelDesc &d = P->lv[l];
        d.img_rows = lr[l]; d.img_cols = lc[l];
        if (d.img_rows < 4 || d.img_cols < 4) {
            snprintf(buf, sizeof buf, "pyramid level %d is %dx%d", l, lr[l], lc[l]);
            err = buf;
            return PBD_ERR_INVALID;
        }
        d.blk_cols = (int)roundf((float)lc[l] / (float)sbin);   // HOGFeatures.cpp:174
        d.blk_rows = (int)roundf((float)lr[l] / (float)sbin);
        d.cols = std::max(d.blk_cols - 2, 0);
        d.rows = std::max(d.blk_rows - 2, 0);
        d.src_level = l >= interval ? l - interval : -1;
        d.img_off = pix; d.blk_off = blk; d.cell_off = cell;
        d.tab_x = d.tab_y = 0;
        pix += (long long)lr[l] * lc[l];
        blk += (long long)d.blk_rows * d.blk_cols;
        cell += (long long)d.rows * d.cols;
        if (l == interval - 1) P->npix_resized = pix;
        if (l < interval) {
            // cv::resize INTER_LINEAR 8U coefficient tables (OpenCV imgwarp.cpp)
            const double scale_x = 1. / ((double)lc[l] / cols), scale_y = 1. / ((double)lr[l] / rows);
            d.tab_x = (int)tabx.size();
            d.tab_y = (int)taby.size();
            for (int dx = 0; dx < lc[l]; ++dx) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = (int)floorf(fx);
                fx -= (float)sx;
                if (sx < 0) { fx = 0; sx = 0; }
                const int last = sx >= cols - 1;
                if (last) { fx = 0; sx = cols - 1; }
                tabx.push_back({sx, sat_short_round((1.f - fx) * 2048), sat_short_round(fx * 2048)});
                tabxf.push_back({sx, last, 1.f - fx, fx});
            }
            for (int dy = 0; dy < lr[l]; ++dy) {
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                int sy = (int)floorf(fy);
                fy -= (float)sy;
                const int y0 = std::min(std::max(sy, 0), rows - 1), y1 = std::min(std::max(sy + 1, 0), rows - 1);
                taby.push_back({y0, y1, sat_short_round((1.f - fy) * 2048), sat_short_round(fy * 2048)});
                tabyf.push_back({y0, y1, 1.f - fy, fy});
            }
        }
    }
    P->pix_per_frame = pix; P->blk_per_frame = blk; P->cell_per_frame = cell;
    if (P->npix_resized == 0) P->npix_resized = pix;
    P->htabx = std::move(tabx); P->htaby = std::move(taby); P->htabxf = std::move(tabxf); P->htabyf = std::move(tabyf);
    return PBD_OK;
}

// the HOG coordinate table grows with the largest frame seen
int grow_coord(pbd_handle *h, int rows, int cols)
{
    const int need = std::max(rows, cols) + 4 * h->sbin + 8;
    if (need > h->coord_n) {
        // HOGFeatures.cpp:252-259: yp = ((T)y+0.5)/(T)sbin - 0.5; iyp = floor(yp); vy0 = yp-iyp; vy1 = 1.0-vy0
        if (h->f64) {
            std::vector<HogCoordD> coord(need);
            for (int t = 0; t < need; ++t) {
                const double tp = ((double)t + 0.5) / (double)h->sbin - 0.5;
                const int ip = (int)floor(tp);
                const double v0 = tp - (double)ip;
                coord[t] = {ip, v0, 1.0 - v0};
            }
            HIPCHK(h, h->d_coord.ensure(coord.size() * sizeof(HogCoordD)));
            HIPCHK(h, hipMemcpy(h->d_coord.p, coord.data(), coord.size() * sizeof(HogCoordD), hipMemcpyHostToDevice));
        } else {
            std::vector<HogCoord> coord(need);
            for (int t = 0; t < need; ++t) {
                const float tp = (float)(((double)(float)t + 0.5) / (double)(float)h->sbin - 0.5);
                const int ip = (int)floorf(tp);
                const float v0 = tp - (float)ip;
                const float v1 = (float)(1.0 - (double)v0);
                coord[t] = {ip, v0, v1};
            }
            HIPCHK(h, h->d_coord.ensure(coord.size() * sizeof(HogCoord)));
            HIPCHK(h, hipMemcpy(h->d_coord.p, coord.data(), coord.size() * sizeof(HogCoord), hipMemcpyHostToDevice));
        }
        h->coord_n = need;
    }
    return PBD_OK;
}

int get_image_plan(pbd_handle *h, int rows, int cols, Plan **out)
{
    for (auto &p : h->plans)
        if (p->kind == 0 && p->rows == rows && p->cols == cols) { *out = p.get(); return PBD_OK; }
    auto P = std::make_unique<Plan>();
    {
        std::string err;
        if (int rc = image_plan_host(rows, cols, h->sbin, h->interval, *P, err)) return fail(h, rc, "%s", err.c_str());
    }
    const int n = P->nlevels;
    long long blk = P->blk_per_frame, cell = P->cell_per_frame;
    if (h->shard_world > 1) {
        // Level sharding (secondary partitioning): levels are independent through HOG, convolution and DP, so
        // one frame can be split over GPUs by giving each a subset of the levels.  Longest-processing-time assignment
        // over the cell counts (level 0 alone is 13 % of a VGA frame): levels by decreasing size, each to the rank
        // with the least work so far.  Levels of other ranks keep their pyramid image here (a pyrDown chain may run
        // through them) but get empty block / feature maps, so every later stage skips them.
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return (long long)P->lv[a].rows * P->lv[a].cols > (long long)P->lv[b].rows * P->lv[b].cols;
        });
        std::vector<long long> load(h->shard_world, 0);
        std::vector<int> owner(n, 0);
        for (int l : order) {
            const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            owner[l] = r;
            load[r] += (long long)P->lv[l].rows * P->lv[l].cols;
        }
        blk = 0; cell = 0;
        for (int l = 0; l < n; ++l) {
            LevelDesc &d = P->lv[l];
            if (owner[l] != h->shard_rank) d.blk_rows = d.blk_cols = d.rows = d.cols = 0;
            d.blk_off = blk; d.cell_off = cell;
            blk += (long long)d.blk_rows * d.blk_cols;
            cell += (long long)d.rows * d.cols;
        }
    }
    P->blk_per_frame = blk; P->cell_per_frame = cell;
    HIPCHK(h, P->d_tabx.upload(P->htabx));
    HIPCHK(h, P->d_taby.upload(P->htaby));
    HIPCHK(h, P->d_tabxf.upload(P->htabxf));
    HIPCHK(h, P->d_tabyf.upload(P->htabyf));
    HIPCHK(h, finish_plan_tables(*P, h->sbin));
    if (int rc = grow_coord(h, rows, cols)) return rc;
    *out = P.get();
    cache_plan(h, std::move(P));
    return PBD_OK;
}

int get_dims_plan(pbd_handle *h, int nlevels, const int *rows, const int *cols, Plan **out)
{
    if (nlevels <= 0 || nlevels > PBD_MAX_LEVELS) return fail(h, PBD_ERR_INVALID, "nlevels %d out of range", nlevels);
    std::vector<int> key;
    for (int l = 0; l < nlevels; ++l) {
        if (rows[l] < 0 || cols[l] < 0 || rows[l] > 32000 || cols[l] > 32000)
            return fail(h, PBD_ERR_INVALID, "level %d size %dx%d out of range", l, rows[l], cols[l]);
        key.push_back(rows[l]); key.push_back(cols[l]);
    }
    for (auto &p : h->plans)
        if (p->kind == 1 && p->key_dims == key) { *out = p.get(); return PBD_OK; }
    auto P = std::make_unique<Plan>();
    P->kind = 1; P->key_dims = key; P->nlevels = nlevels; P->interval = h->interval;
    P->lv.resize(nlevels);
    P->scales.assign(nlevels, 1.f);
    long long cell = 0;
    for (int l = 0; l < nlevels; ++l) {
        LevelDesc &d = P->lv[l];
        memset(&d, 0, sizeof d);
        d.rows = rows[l]; d.cols = cols[l]; d.src_level = -1; d.cell_off = cell;
        cell += (long long)rows[l] * cols[l];
    }
    P->cell_per_frame = cell;
    HIPCHK(h, finish_plan_tables(*P, h->sbin));
    *out = P.get();
    cache_plan(h, std::move(P));
    return PBD_OK;
}

// ---- mixed-size plans ----------------------------------------------------------------------------
// Appends frame Q (an unsharded image plan) to the virtual frame M: its levels, scales and resize tables, with every offset
// shifted past the frames already in M.  Host only.
void mixed_append(Plan &M, const Plan &Q)
{
    const int lv0 = M.nlevels, f = M.mixed_frames;
    const int tx0 = (int)M.htabx.size(), ty0 = (int)M.htaby.size();
    if (M.frame_lv0.empty()) M.frame_lv0.push_back(0);
    for (int l = 0; l < Q.nlevels; ++l) {
        LevelDesc d = Q.lv[l];
        d.img_off += M.pix_per_frame; d.blk_off += M.blk_per_frame; d.cell_off += M.cell_per_frame;
        if (d.src_level >= 0) d.src_level += lv0;
        else { d.tab_x += tx0; d.tab_y += ty0; }
        M.lv.push_back(d);
        M.scales.push_back(Q.scales[l]);
        M.lv_frame.push_back(f);
        M.lv_local.push_back(l);
    }
    M.htabx.insert(M.htabx.end(), Q.htabx.begin(), Q.htabx.end());
    M.htaby.insert(M.htaby.end(), Q.htaby.begin(), Q.htaby.end());
    M.htabxf.insert(M.htabxf.end(), Q.htabxf.begin(), Q.htabxf.end());
    M.htabyf.insert(M.htabyf.end(), Q.htabyf.begin(), Q.htabyf.end());
    M.nlevels += Q.nlevels;
    M.pix_per_frame += Q.pix_per_frame; M.blk_per_frame += Q.blk_per_frame; M.cell_per_frame += Q.cell_per_frame;
    M.frame_lv0.push_back(M.nlevels);
    M.fdim.push_back(make_int2(Q.rows, Q.cols));
    M.key_dims.push_back(Q.rows); M.key_dims.push_back(Q.cols);
    M.mixed_frames += 1;
}

void post_canvas_plan(Plan &M);

// After the last mixed_append: the pyramid launches (every frame's resized levels in one, then one per octave over every frame)
// and the post-processing tables.  Host only.
void mixed_finish(Plan &M, int interval)
{
    M.kind = 2; M.interval = interval;
    M.npix_resized = 0;
    int octaves = 0;
    for (int f = 0; f < M.mixed_frames; ++f)
        octaves = std::max(octaves, (M.frame_lv0[f + 1] - M.frame_lv0[f] + interval - 1) / interval);
    for (int k = 0; k < octaves; ++k) {
        M.run_lev0.push_back((int)M.run_lev.size());
        M.run_off0.push_back((long long)M.run_off.size());
        long long pix = 0;
        int n = 0;
        for (int f = 0; f < M.mixed_frames; ++f)
            for (int l = M.frame_lv0[f] + k * interval; l < std::min(M.frame_lv0[f] + (k + 1) * interval, M.frame_lv0[f + 1]); ++l) {
                M.run_lev.push_back(l);
                M.run_off.push_back(pix);
                pix += (long long)M.lv[l].img_rows * M.lv[l].img_cols;
                ++n;
            }
        M.run_off.push_back(pix);
        M.run_n.push_back(n);
        M.run_npix.push_back(pix);
    }
    post_canvas_plan(M);
}

// the suppression stage's per-frame tables of a list of frame sizes (M.fdim, M.mixed_frames): each frame's canvas in LDS or at
// its offset in the global workspace.  Host only.
void post_canvas_plan(Plan &M)
{
    M.fcanvas.assign(M.mixed_frames, 0);
    M.post_lds.clear(); M.post_glb.clear();
    M.post_lds_words = M.post_glb_words = 0;
    for (int f = 0; f < M.mixed_frames; ++f) {
        const int r = M.fdim[f].x, c = M.fdim[f].y;
        if (post_canvas_in_lds(r, c)) {
            M.post_lds.push_back(f);
            M.post_lds_words = std::max(M.post_lds_words, post_canvas_words(r, c));
        } else {
            M.post_glb.push_back(f);
            M.fcanvas[f] = (long long)M.post_glb_words;
            M.post_glb_words += post_canvas_words(r, c);
        }
    }
}

// the mixed plan of one call's frame sizes (rows[f] x cols[f], call order), built from the cached image plans of its sizes
int get_mixed_plan(pbd_handle *h, int nframes, const int *rows, const int *cols, Plan **out)
{
    std::vector<int> key;
    for (int f = 0; f < nframes; ++f) { key.push_back(rows[f]); key.push_back(cols[f]); }
    for (auto &p : h->plans)
        if (p->kind == 2 && p->key_dims == key) { *out = p.get(); return PBD_OK; }
    auto M = std::make_unique<Plan>();
    // every frame's tables: those of a cached image plan of its size, else built on the host only (a mixed call never uses an
    // image plan's device tables, and sizes seen only here do not take the equal-size path's places in the plan cache)
    std::map<std::pair<int, int>, std::unique_ptr<Plan>> built;
    for (int f = 0; f < nframes; ++f) {
        const Plan *Q = nullptr;
        for (auto &p : h->plans)
            if (p->kind == 0 && p->rows == rows[f] && p->cols == cols[f]) { Q = p.get(); break; }
        if (!Q) {
            std::unique_ptr<Plan> &B = built[std::make_pair(rows[f], cols[f])];
            if (!B) {
                B = std::make_unique<Plan>();
                std::string err;
                if (int rc = image_plan_host(rows[f], cols[f], h->sbin, h->interval, *B, err))
                    return fail(h, rc, "frame %d: %s", f, err.c_str());
            }
            Q = B.get();
        }
        mixed_append(*M, *Q);
    }
    for (int f = 0; f < nframes; ++f)
        if (int rc = grow_coord(h, rows[f], cols[f])) return rc;
    mixed_finish(*M, h->interval);
    HIPCHK(h, M->d_tabx.upload(M->htabx));
    HIPCHK(h, M->d_taby.upload(M->htaby));
    HIPCHK(h, M->d_tabxf.upload(M->htabxf));
    HIPCHK(h, M->d_tabyf.upload(M->htabyf));
    HIPCHK(h, M->d_lv_frame.upload(M->lv_frame));
    HIPCHK(h, M->d_lv_local.upload(M->lv_local));
    HIPCHK(h, M->d_run_lev.upload(M->run_lev));
    HIPCHK(h, M->d_run_off.upload(M->run_off));
    HIPCHK(h, M->d_fdim.upload(M->fdim));
    HIPCHK(h, M->d_fcanvas.upload(M->fcanvas));
    HIPCHK(h, M->d_post_lds.upload(M->post_lds));
    HIPCHK(h, M->d_post_glb.upload(M->post_glb));
    HIPCHK(h, finish_plan_tables(*M, h->sbin));
    *out = M.get();
    cache_plan(h, std::move(M));
    return PBD_OK;
}

// IEEE binary16 <-> float on the host (round to nearest even, what v_cvt_f16_f32 does)
uint16_t host_f2h(float f)
{
    uint32_t u; memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t ax = u & 0x7fffffffu;
    if (ax > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // rounds to >= 65520: inf
    if (ax < 0x33000001u) return sign;                                       // below half the smallest subnormal: 0
    const int e = (int)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7fffffu) | 0x800000u;
    int shift = e >= -14 ? 13 : 13 + (-14 - e);                              // bits dropped from the 24-bit significand
    const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1);
    uint32_t q = m >> shift;
    if (rest > half || (rest == half && (q & 1u))) ++q;
    const uint32_t bits = e >= -14 ? (((uint32_t)(e + 15) << 10) + (q - 0x400u)) : q;   // carry propagates into the exponent
    return (uint16_t)(sign | bits);
}
float host_h2f(uint16_t hv)
{
    const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16;
    const uint32_t ex = (hv >> 10) & 0x1fu, man = hv & 0x3ffu;
    uint32_t u;
    if (ex == 0x1f) u = sign | 0x7f800000u | (man << 13);
    else if (ex != 0) u = sign | ((ex + 112u) << 23) | (man << 13);
    else if (man == 0) u = sign;
    else {                                                                   // subnormal half: normalise
        int sh = 0;
        uint32_t mm = man;
        while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
        u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f; memcpy(&f, &u, 4);
    return f;
}

// ---- model tables --------------------------------------------------------------------------------
// Work items of k_conv3: the nf filters of a size class cut into units of 8 / 6 (and at most one of 4 or 2) filters so that
// `nw` waves taking units largest-first finish together.  156 filters, 6 waves: 6 x 8 + 18 x 6 -- every wave 8 + 6 + 6 + 6.
void conv_units(int nf, int nw, std::vector<int> &f0, std::vector<int> &ql)
{
    const int P = (nf + 1) / 2;                            // filter pairs (an odd bank ends in a padding lane)
    double best = 1e30;
    int ba = 0, bb = 0, bc = 0;
    for (int a = P / 4; a >= 0; --a)
        for (int c = 0; c <= 2; ++c) {                     // c pairs in one last small unit (0: none)
            const int rest = P - 4 * a - c;
            if (rest < 0 || rest % 3) continue;
            const int b = rest / 3;
            // largest-first hand-out to nw equally fast waves; a unit costs its pairs + a fixed overhead (window reads, stores)
            std::vector<double> load(nw, 0.0);
            auto give = [&](int n, double cost) { for (int i = 0; i < n; ++i) *std::min_element(load.begin(), load.end()) += cost; };
            give(a, 4 + 0.2); give(b, 3 + 0.2); if (c) give(1, c + 0.2);
            const double span = *std::max_element(load.begin(), load.end()) + (c ? 0.01 : 0.0);    // ties: no small unit
            if (span < best - 1e-9) { best = span; ba = a; bb = b; bc = c; }
        }
    f0.clear(); ql.clear();
    int f = 0;
    for (int i = 0; i < ba; ++i) { f0.push_back(f); ql.push_back(8); f += 8; }
    for (int i = 0; i < bb; ++i) { f0.push_back(f); ql.push_back(6); f += 6; }
    if (bc) { f0.push_back(f); ql.push_back(2 * bc); f += 2 * bc; }
}

template <typename R>
int upload_filters_t(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    if (nfilters <= 0) return fail(h, PBD_ERR_INVALID, "no filters");
    for (int f = 0; f < nfilters; ++f)
        if (ksize[f] < 1 || ksize[f] > kConvMaxK) return fail(h, PBD_ERR_UNSUPPORTED, "filter %d: size %d not supported (1..%d)", f, ksize[f], kConvMaxK);
    // size classes in order of first appearance
    std::vector<int> sizes;
    for (int f = 0; f < nfilters; ++f)
        if (std::find(sizes.begin(), sizes.end(), ksize[f]) == sizes.end()) sizes.push_back(ksize[f]);
    const int K = ksize[0];
    const bool fast = (sizeof(R) == 4 && K == 5 && sizes.size() == 1);
    const bool mfma = h->cfg.conv_mode == PBD_CONV_MFMA || h->cfg.conv_mode == PBD_CONV_MFMA_F16;
    if (mfma && !fast) return fail(h, PBD_ERR_UNSUPPORTED, "PBD_CONV_MFMA / PBD_CONV_MFMA_F16 need 5x5 filters and PBD_REAL_F32");
    // The new bank is built beside the old one and moved in only when every upload has succeeded: a failed setFilters()
    // (out of memory, an unsupported size) leaves the handle with its previous, complete bank.
    std::vector<pbd_handle::ConvClass> classes(sizes.size());
    DevBuf wrec;
    for (size_t ci = 0; ci < sizes.size(); ++ci) {
        pbd_handle::ConvClass &C = classes[ci];
        C.K = sizes[ci];
        std::vector<int> ids;
        for (int f = 0; f < nfilters; ++f) if (ksize[f] == C.K) ids.push_back(f);
        C.nf = (int)ids.size();
        C.Fpad = (C.nf + kConvQ - 1) / kConvQ * kConvQ;
        // device layout: float 5x5 kernel [group][channel][tap][8] (800 contiguous bytes per (group, channel));
        // generic kernel (other sizes, T=double) [channel][tap][Fpad]
        const bool fast5 = (sizeof(R) == 4 && C.K == 5);
        const int KK = C.K * C.K;
        std::vector<R> w((size_t)32 * KK * C.Fpad, (R)0);
        for (int fl = 0; fl < C.nf; ++fl) {
            const R *src = static_cast<const R *>(filters[ids[fl]]);
            for (int t = 0; t < KK; ++t)
                for (int c = 0; c < 32; ++c) {
                    const R v = src[(size_t)t * 32 + c];
                    if (fast5) w[(((size_t)(fl / kConvQ) * 32 + c) * KK + t) * kConvQ + (fl % kConvQ)] = v;
                    else w[((size_t)c * KK + t) * C.Fpad + fl] = v;
                }
        }
        HIPCHK(h, C.wts.ensure(w.size() * sizeof(R)));
        HIPCHK(h, hipMemcpy(C.wts.p, w.data(), w.size() * sizeof(R), hipMemcpyHostToDevice));
        if (sizes.size() > 1) HIPCHK(h, C.fmap.upload(ids));
        if (fast5) {
            std::vector<int> uf0, uql;
            conv_units(C.nf, kConv3NW, uf0, uql);
            C.nunits = (int)uf0.size();
            std::vector<int> uoff(C.nunits, 0);
            size_t tot = 0;
            for (int u = 0; u < C.nunits; ++u) { uoff[u] = (int)tot; tot += (size_t)32 * KK * uql[u]; }
            std::vector<float> w3(tot + 16, 0.0f);       // (slack: the last tap row is fetched once more past the last channel)
            for (int u = 0; u < C.nunits; ++u)
                for (int q = 0; q < uql[u] && uf0[u] + q < C.nf; ++q) {
                    const R *src = static_cast<const R *>(filters[ids[uf0[u] + q]]);
                    for (int t = 0; t < KK; ++t)
                        for (int c = 0; c < 32; ++c) w3[uoff[u] + ((size_t)c * KK + t) * uql[u] + q] = (float)src[(size_t)t * 32 + c];
                }
            HIPCHK(h, C.unit_woff.upload(uoff));
            // channel 31 of a window that leaves the image: the reference's sum over the out-of-image taps (border value 1,
            // src/SpatialConvolutionEngine.cpp:147-156) in its tap order (raster, zero weights skipped: src/filter.cpp:3818-3856,
            // 3916-3922), for every combination of rows / columns outside at the top, bottom, left and right (0..2 each)
            C.c31stride = (C.nf + 15) & ~7;                     // a unit's 8 consecutive entries stay inside the row
            std::vector<float> tab((size_t)81 * C.c31stride, 0.0f);
            for (int cs = 0; cs < 81; ++cs) {
                const int right = cs % 3, left = cs / 3 % 3, bot = cs / 9 % 3, top = cs / 27;
                for (int fl = 0; fl < C.nf; ++fl) {
                    const R *src = static_cast<const R *>(filters[ids[fl]]);
                    float sum = 0.0f;
                    for (int i = 0; i < 5; ++i)
                        for (int j = 0; j < 5; ++j) {
                            if (!(i < top || i > 4 - bot || j < left || j > 4 - right)) continue;
                            const float w = (float)src[(size_t)(i * 5 + j) * 32 + 31];
                            if (w != 0.0f) sum = sum + w;
                        }
                    tab[(size_t)cs * C.c31stride + fl] = sum;
                }
            }
            HIPCHK(h, C.c31tab.upload(tab));
            HIPCHK(h, C.wts3.ensure(w3.size() * sizeof(float)));
            HIPCHK(h, hipMemcpy(C.wts3.p, w3.data(), w3.size() * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(h, C.unit_f0.upload(uf0));
            HIPCHK(h, C.unit_ql.upload(uql));
        }
        if (h->cfg.conv_mode == PBD_CONV_MFMA_F64) {
            // A-fragments in the order k_conv_mfma_f64 reads them.  Pass ps (M-tiles [m0, m1)), channel block cb, tap, q-pair qp,
            // M-tile m, q of the pair e, lane l: filter (m0 + m) * 16 + (l & 15), channel cb * CB + (l >> 4) * QN + qp * QS + e
            // (lane group g supplies channels g QN .. g QN + QN - 1 of its cell); filters past nf are zero
            const int QN = conv_mfma_f64_qn(C.K), CB = 4 * QN, QS = std::min(QN, 2), QP = QN / QS;
            const int mtiles = (C.nf + 15) / 16, passes = f64_passes(mtiles);
            std::vector<double> wf((size_t)mtiles * 8 * KK * 64, 0.0);
            size_t o = 0;
            for (int ps = 0; ps < passes; ++ps) {
                const int m0 = f64_pass_begin(ps, mtiles, passes), mb = f64_pass_begin(ps + 1, mtiles, passes) - m0;
                for (int cb = 0; cb < 32 / CB; ++cb)
                    for (int t = 0; t < KK; ++t)
                        for (int qp = 0; qp < QP; ++qp)
                            for (int m = 0; m < mb; ++m)
                                for (int e = 0; e < QS; ++e)
                                    for (int l = 0; l < 64; ++l, ++o) {
                                        const int fl = (m0 + m) * 16 + (l & 15);
                                        const int c = cb * CB + (l >> 4) * QN + qp * QS + e;
                                        if (fl < C.nf) wf[o] = (double)static_cast<const R *>(filters[ids[fl]])[(size_t)t * 32 + c];
                                    }
            }
            HIPCHK(h, C.wfrag64.ensure(wf.size() * sizeof(double)));
            HIPCHK(h, hipMemcpy(C.wfrag64.p, wf.data(), wf.size() * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    const int Fpad = (nfilters + kConvQ - 1) / kConvQ * kConvQ;
    if (mfma) {
        const bool f16 = h->cfg.conv_mode == PBD_CONV_MFMA_F16;
        // bf16 mode: x = hi + lo with round-to-nearest-even; fp16 mode: one rounding
        auto f2bf = [](float f) -> uint16_t {
            uint32_t u; memcpy(&u, &f, 4);
            if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
            u += 0x7fffu + ((u >> 16) & 1u);
            return (uint16_t)(u >> 16);
        };
        auto bf2f = [](uint16_t b) -> float { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
        // A-operand fragments in the order the kernel consumes them: [pass][tap][k-step][M-tile][hi|lo][lane] x 8 values.
        // Lane (r = lane & 31, hh = lane >> 5) of v_mfma_f32_32x32x16 holds row r (filter), k = hh*8 .. hh*8+7 (channels)
        const int NV = f16 ? 1 : 2, MT = kMfmaFilterBlock / 32;
        const int passes = (nfilters + kMfmaFilterBlock - 1) / kMfmaFilterBlock;
        std::vector<uint16_t> rec((size_t)passes * K * K * 2 * MT * NV * 64 * 8, 0);
        for (int ps = 0; ps < passes; ++ps)
            for (int t = 0; t < K * K; ++t)
                for (int kh = 0; kh < 2; ++kh)
                    for (int mt = 0; mt < MT; ++mt)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int f = ps * kMfmaFilterBlock + mt * 32 + (lane & 31);
                            if (f >= nfilters) continue;
                            const float *src = reinterpret_cast<const float *>(filters[f]) + (size_t)t * 32 + kh * 16 + (lane >> 5) * 8;
                            const size_t base = (((((size_t)ps * K * K + t) * 2 + kh) * MT + mt) * NV) * 64 * 8;
                            for (int j = 0; j < 8; ++j) {
                                const float v = src[j];
                                if (f16) { rec[base + (size_t)lane * 8 + j] = host_f2h(v); continue; }
                                const uint16_t hi = f2bf(v);
                                rec[base + (size_t)lane * 8 + j] = hi;
                                rec[base + (size_t)(64 + lane) * 8 + j] = f2bf(v - bf2f(hi));
                            }
                        }
        HIPCHK(h, wrec.ensure(rec.size() * 2));
        HIPCHK(h, hipMemcpy(wrec.p, rec.data(), rec.size() * 2, hipMemcpyHostToDevice));
    }
    // commit
    h->conv_classes = std::move(classes);
    if (mfma) h->d_wrec = std::move(wrec);
    h->F = nfilters; h->Fpad = Fpad; h->ksize = K;
    h->filter_ksize.assign(ksize, ksize + nfilters);
    h->filters_set = true;
    return PBD_OK;
}

int upload_filters(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    return h->f64 ? upload_filters_t<double>(h, nfilters, filters, ksize) : upload_filters_t<float>(h, nfilters, filters, ksize);
}

// After pbd_conv_set_filters replaced the bank: the model tables built by build_model index response planes by
// filter id, and the part boxes of argmin use the filter size (include/Parts.hpp:185-187), so both are re-checked /
// rebuilt against the new bank.  A bank that does not cover the model's ids leaves the convolution engine usable on
// its own (IConvolutionEngine::pdf) and makes the model-dependent calls fail with PBD_ERR_STATE.
int revalidate_bank(pbd_handle *h)
{
    h->bank_matches_model = true;
    for (int f : h->filterid)
        if (f < 0 || f >= h->F) { h->bank_matches_model = false; return PBD_OK; }
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        for (int p = 0; p < np; ++p) {
            PartWalk &w = h->walk[h->walk_off[c] + p];
            const int K = h->mix_offset[p0 + p + 1] - h->mix_offset[p0 + p];
            for (int mm = 0; mm < K; ++mm) w.ksize[mm] = h->filter_ksize[h->filterid[h->mix_offset[p0 + p] + mm]];
        }
    }
    HIPCHK(h, h->d_walk.upload(h->walk));
    return PBD_OK;
}

int build_model(pbd_handle *h, const pbd_model *m)
{
    if (m->flen != 32 || m->norient != 18)
        return fail(h, PBD_ERR_UNSUPPORTED, "flen %d / norient %d: only 32 / 18 are supported", m->flen, m->norient);
    if (m->ncomponents < 1 || m->nfilters < 1 || m->sbin < 2 || m->interval < 1)
        return fail(h, PBD_ERR_INVALID, "bad model header");
    h->NC = m->ncomponents; h->sbin = m->sbin; h->interval = m->interval; h->norient = m->norient;
    h->thresh = m->thresh;
    const int totparts = m->part_offset[m->ncomponents];
    const int totmix = m->mix_offset[totparts];
    h->part_offset.assign(m->part_offset, m->part_offset + m->ncomponents + 1);
    h->parentid.assign(m->parentid, m->parentid + totparts);
    h->mix_offset.assign(m->mix_offset, m->mix_offset + totparts + 1);
    h->filterid.assign(m->filterid, m->filterid + totmix);
    h->biasid.assign(m->biasid, m->biasid + totmix);
    h->defid.assign(m->defid, m->defid + totmix);
    h->biasw.assign(m->biasw, m->biasw + m->nbias);
    h->defw.assign(m->defw, m->defw + (size_t)m->ndefs * 4);
    h->anchors.assign(m->anchors, m->anchors + (size_t)m->ndefs * 2);

    // filters
    {
        if (h->f64 ? !m->filters_f64 : !m->filters_f32) return fail(h, PBD_ERR_INVALID, "model has no filters of the requested real type");
        std::vector<const void *> fp(m->nfilters);
        for (int f = 0; f < m->nfilters; ++f)
            fp[f] = h->f64 ? static_cast<const void *>(m->filters_f64 + m->filter_offset[f])
                           : static_cast<const void *>(m->filters_f32 + m->filter_offset[f]);
        if (int rc = upload_filters(h, m->nfilters, fp.data(), m->filter_ksize)) return rc;
    }

    // validation + pointer slots + depth
    h->ptr_slot.assign(totparts, 0);
    std::vector<int> depth(totparts, 0);
    int NS = 0, maxdepth = 0;
    h->max_parts = 0;
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        if (np < 1) return fail(h, PBD_ERR_INVALID, "component %d has no parts", c);
        h->max_parts = std::max(h->max_parts, np);
        std::set<int> seen;
        for (int p = 0; p < np; ++p) {
            const int gp = p0 + p, par = h->parentid[gp];
            const int K = h->mix_offset[gp + 1] - h->mix_offset[gp];
            if (K < 1 || K > kMaxMix) return fail(h, PBD_ERR_UNSUPPORTED, "part %d has %d mixtures (1..%d supported)", p, K, kMaxMix);
            h->max_mix = std::max(h->max_mix, K);
            if ((p == 0) != (par < 0) || par >= p) return fail(h, PBD_ERR_INVALID, "part %d: parent %d breaks topological order", p, par);
            for (int mm = 0; mm < K; ++mm) {
                const int f = h->filterid[h->mix_offset[gp] + mm];
                if (f < 0 || f >= h->F) return fail(h, PBD_ERR_INVALID, "filter id %d out of range", f);
                if (!seen.insert(f).second) h->seq_mode = true;   // accumulators keyed by filter id interact: see below
            }
            h->ptr_slot[gp] = NS;
            if (p > 0) {
                const int gpar = p0 + par;
                const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                NS += L;
                depth[gp] = depth[gpar] + 1;
                maxdepth = std::max(maxdepth, depth[gp]);
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm;
                    const int d = h->defid[gm], b = h->biasid[gm];
                    if (d < 0 || d >= m->ndefs) return fail(h, PBD_ERR_INVALID, "defid %d out of range", d);
                    if (b < 0 || b + L > m->nbias) return fail(h, PBD_ERR_INVALID, "biasid %d out of range", b);
                    if (h->defw[(size_t)d * 4 + 0] == 0.f || h->defw[(size_t)d * 4 + 2] == 0.f)
                        return fail(h, PBD_ERR_INVALID, "deformation %d has a zero quadratic term", d);
                }
            } else {
                const int b = h->biasid[h->mix_offset[gp]];
                if (b < 0 || b >= m->nbias) return fail(h, PBD_ERR_INVALID, "root biasid %d out of range", b);
            }
        }
    }
    if (h->max_parts > kWalkMaxParts) return fail(h, PBD_ERR_UNSUPPORTED, "%d parts per component (max %d)", h->max_parts, kWalkMaxParts);
    h->NS = NS;

    // children (descending index) per part
    std::vector<std::vector<int>> children(totparts);
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        for (int p = np - 1; p > 0; --p) children[p0 + h->parentid[p0 + p]].push_back(p0 + p);
    }

    h->groups.clear();
    h->JGmax = 0;
    h->NM = totmix;
    h->totmix = totmix;
    auto dt_job = [&](int gm, bool from_acc, int plane) {
        DtJob j{};
        j.from_acc = from_acc ? 1 : 0;
        j.plane = plane;
        j.gm = gm;
        const int d = h->defid[gm];
        const float *w = &h->defw[(size_t)d * 4];
        j.ax = (double)(-w[0]); j.bx = (double)(-w[1]); j.ay = (double)(-w[2]); j.by = (double)(-w[3]);
        j.osx = h->anchors[(size_t)d * 2]; j.osy = h->anchors[(size_t)d * 2 + 1];
        return j;
    };
    std::vector<std::vector<char>> touched(h->NC, std::vector<char>(h->F, 0));   // sequential schedule: accumulator (c, f) exists
    if (h->seq_mode) {
        // The reference's own order (src/DynamicProgram.cpp:95): parts nparts-1 .. 1, one step per part; the
        // accumulated scores live in planes keyed by (component, filter id) as its `ncscores` (:93,115-119,154-156).
        // Step s takes part np-1-s of every component (components are independent).
        h->NM = h->NC * h->F;
        for (int sidx = 0; sidx + 1 < h->max_parts; ++sidx) {
            Group g;
            for (int c = 0; c < h->NC; ++c) {
                const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
                const int p = np - 1 - sidx;
                if (p < 1) continue;
                const int gp = p0 + p, gpar = p0 + h->parentid[gp];
                const int K = h->mix_offset[gp + 1] - h->mix_offset[gp], L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                SeqCombineJob sj{};
                sj.job_begin = (int)g.jobs.size(); sj.nmix = K; sj.slot = h->ptr_slot[gp]; sj.npar = L;
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm, f = h->filterid[gm];
                    g.jobs.push_back(dt_job(gm, touched[c][f] != 0, touched[c][f] ? c * h->F + f : f));   // score_in, :115-119
                    sj.bias_off[mm] = h->biasid[gm];
                }
                for (int pm = 0; pm < L; ++pm) {
                    const int fp = h->filterid[h->mix_offset[gpar] + pm];
                    sj.target[pm] = c * h->F + fp; sj.filter[pm] = fp;
                    sj.init[pm] = touched[c][fp] ? 0 : 1;
                    touched[c][fp] = 1;
                }
                g.sjobs.push_back(sj);
            }
            h->JGmax = std::max(h->JGmax, (int)g.jobs.size());
            h->groups.push_back(std::move(g));
        }
    }
    // depth groups, deepest first: DT jobs of the parts at depth `dep`, combine jobs of their parents
    for (int dep = h->seq_mode ? 0 : maxdepth; dep >= 1; --dep) {
        Group g;
        std::vector<int> job_begin_of(totparts, -1);
        for (int c = 0; c < h->NC; ++c) {
            const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
            for (int p = 1; p < np; ++p) {
                const int gp = p0 + p;
                if (depth[gp] != dep) continue;
                const int K = h->mix_offset[gp + 1] - h->mix_offset[gp];
                job_begin_of[gp] = (int)g.jobs.size();
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm;
                    g.jobs.push_back(dt_job(gm, !children[gp].empty(), children[gp].empty() ? h->filterid[gm] : gm));
                }
            }
            // parents at depth dep-1 whose children (all at depth dep) were just listed
            for (int p = 0; p < np; ++p) {
                const int gpar = p0 + p;
                if (depth[gpar] != dep - 1 || children[gpar].empty()) continue;
                const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                CombineJob cj{};
                cj.npar = L; cj.acc_plane = h->mix_offset[gpar];
                for (int pm = 0; pm < L; ++pm) cj.filter[pm] = h->filterid[h->mix_offset[gpar] + pm];
                cj.child_begin = (int)g.childs.size();
                for (int ch : children[gpar]) {   // already in descending index order
                    ChildDesc cd{};
                    cd.job_begin = job_begin_of[ch];
                    cd.nmix = h->mix_offset[ch + 1] - h->mix_offset[ch];
                    cd.slot = h->ptr_slot[ch];
                    for (int mm = 0; mm < cd.nmix; ++mm) cd.bias_off[mm] = h->biasid[h->mix_offset[ch] + mm];
                    g.childs.push_back(cd);
                }
                cj.child_end = (int)g.childs.size();
                g.cjobs.push_back(cj);
            }
        }
        h->JGmax = std::max(h->JGmax, (int)g.jobs.size());
        h->groups.push_back(std::move(g));
    }
    for (auto &g : h->groups) {
        HIPCHK(h, g.d_jobs.upload(g.jobs));
        // the usual deformation (w1 = w3 = +0.0f, so b = -0.0): the passes then run without the b terms
        auto neg_zero = [](double v) { return v == 0.0 && std::signbit(v); };
        g.bz_x = g.bz_y = 1;
        for (const DtJob &j : g.jobs) {
            if (!(neg_zero(j.bx) && j.ax != 0.0)) g.bz_x = 0;
            if (!(neg_zero(j.by) && j.ay != 0.0)) g.bz_y = 0;
        }
        HIPCHK(h, g.d_childs.upload(g.childs));
        HIPCHK(h, g.d_cjobs.upload(g.cjobs));
        HIPCHK(h, g.d_sjobs.upload(g.sjobs));
    }
    h->rjobs.assign(h->NC, RootJob{});
    h->walk.clear(); h->walk_off.assign(h->NC + 1, 0);
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        RootJob &r = h->rjobs[c];
        r.nmix = h->mix_offset[p0 + 1] - h->mix_offset[p0];
        r.from_acc = 0;
        for (int mm = 0; mm < r.nmix; ++mm) {
            const int f = h->filterid[h->mix_offset[p0] + mm];
            const bool acc = h->seq_mode ? touched[c][f] != 0 : !children[p0].empty();
            if (acc) r.from_acc |= 1 << mm;
            r.plane[mm] = !acc ? f : h->seq_mode ? c * h->F + f : h->mix_offset[p0] + mm;
        }
        r.bias = h->biasw[h->biasid[h->mix_offset[p0]]];
        h->walk_off[c] = (int)h->walk.size();
        for (int p = 0; p < np; ++p) {
            PartWalk w{};
            w.parent = h->parentid[p0 + p];
            w.slot = h->ptr_slot[p0 + p];
            w.mix0 = h->mix_offset[p0 + p];
            const int K = h->mix_offset[p0 + p + 1] - h->mix_offset[p0 + p];
            for (int mm = 0; mm < K; ++mm) w.ksize[mm] = m->filter_ksize[h->filterid[h->mix_offset[p0 + p] + mm]];
            h->walk.push_back(w);
        }
    }
    h->walk_off[h->NC] = (int)h->walk.size();
    HIPCHK(h, h->d_rjobs.upload(h->rjobs));
    HIPCHK(h, h->d_walk.upload(h->walk));
    HIPCHK(h, h->d_walk_off.upload(h->walk_off));
    HIPCHK(h, h->d_biasw.upload(h->biasw));

    // the model vector (pbd_model_vector) and the strides of an example (pbd_examples*)
    h->nbias = m->nbias; h->ndefs = m->ndefs;
    h->model_ksize.assign(m->filter_ksize, m->filter_ksize + m->nfilters);
    const long long fbase = (long long)m->nbias + 4LL * m->ndefs;
    long long len = fbase;
    h->model_foff.assign(m->nfilters, 0);
    for (int f = 0; f < m->nfilters; ++f) {
        if (m->filter_offset[f] < 0) return fail(h, PBD_ERR_INVALID, "filter %d: negative filter_offset", f);
        h->model_foff[f] = m->filter_offset[f];
        len = std::max(len, fbase + m->filter_offset[f] + (long long)m->filter_ksize[f] * m->filter_ksize[f] * 32);
    }
    if (len > INT32_MAX) return fail(h, PBD_ERR_UNSUPPORTED, "model vector of %lld values (at most 2^31 - 1)", len);
    h->mvec.assign((size_t)len * h->rs, 0);
    auto put = [&](long long o, double v) {
        if (h->f64) reinterpret_cast<double *>(h->mvec.data())[o] = v;
        else reinterpret_cast<float *>(h->mvec.data())[o] = (float)v;
    };
    for (int b = 0; b < m->nbias; ++b) put(b, m->biasw[b]);
    for (long long i = 0; i < 4LL * m->ndefs; ++i) put(m->nbias + i, m->defw[i]);
    for (int f = 0; f < m->nfilters; ++f) {
        const long long n = (long long)m->filter_ksize[f] * m->filter_ksize[f] * 32;
        for (long long i = 0; i < n; ++i)
            put(fbase + m->filter_offset[f] + i, h->f64 ? m->filters_f64[m->filter_offset[f] + i] : (double)m->filters_f32[m->filter_offset[f] + i]);
    }
    h->ex_hdr_words = 4 + 2 * (3 * h->max_parts - 1);
    long long vmax = 0;
    for (int c = 0; c < h->NC; ++c) {
        long long v = 0;
        for (int gp = h->part_offset[c]; gp < h->part_offset[c + 1]; ++gp) {
            int kmax = 0;
            for (int gm = h->mix_offset[gp]; gm < h->mix_offset[gp + 1]; ++gm) kmax = std::max(kmax, m->filter_ksize[h->filterid[gm]]);
            v += 1 + (gp > h->part_offset[c] ? 4 : 0) + (long long)kmax * kmax * 32;
        }
        vmax = std::max(vmax, v);
    }
    if (vmax > INT32_MAX / 2) return fail(h, PBD_ERR_UNSUPPORTED, "an example of %lld values", vmax);
    h->ex_values = (int)((vmax + 3) / 4 * 4);
    return PBD_OK;
}

// ---- stages --------------------------------------------------------------------------------------
// alloc_* size the grow-only workspace for `nframes`; launch_* enqueue the kernels for frames
// [f0, f0+nb) on stream `st` (no allocation, no synchronisation inside).
int alloc_features(pbd_handle *h, Plan &P, int nframes, int cn, int depth)
{
    HIPCHK(h, h->pyr.ensure((size_t)nframes * P.pix_per_frame * cn * depth_size(depth) + 32));   // slack: 8-bit pixels are read with 4- and 16-byte loads
    HIPCHK(h, h->gmag.ensure((size_t)nframes * P.pix_per_frame * h->rs));
    HIPCHK(h, h->gori.ensure((size_t)nframes * P.pix_per_frame + 16));
    HIPCHK(h, h->hist.ensure((size_t)nframes * P.blk_per_frame * 18 * h->rs));
    HIPCHK(h, h->norm.ensure((size_t)nframes * P.blk_per_frame * h->rs));
    HIPCHK(h, h->feat.ensure(std::max<size_t>((size_t)nframes * P.cell_per_frame * 32 * h->rs, 16)));
    return PBD_OK;
}

void launch_hog_stage(pbd_handle *h, Plan &P, int cn, int depth, int f0, int nb, hipStream_t st);

void launch_features(pbd_handle *h, Plan &P, const void *d_frames, int cn, int depth, int f0, int nb, hipStream_t st)
{
    PyrParams pp{};
    pp.lv = P.d_lv.p; pp.nlevels = P.nlevels; pp.interval = std::min(P.interval, P.nlevels); pp.cn = cn; pp.frame0 = f0;
    pp.pix_per_frame = P.pix_per_frame; pp.pyr = h->pyr.as<uint8_t>(); pp.frames = static_cast<const uint8_t *>(d_frames);
    pp.rows = P.rows; pp.cols = P.cols; pp.tabx = P.d_tabx.p; pp.taby = P.d_taby.p;
    pp.depth = depth; pp.tabxf = P.d_tabxf.p; pp.tabyf = P.d_tabyf.p;
    {
        ProfScope ps(h, PBD_K_RESIZE, st);
        launch_resize(pp, nb, P.npix_resized, st);
    }
    for (int first = P.interval; first < P.nlevels; first += P.interval) {
        const int last = std::min(first + P.interval, P.nlevels);
        const long long base = P.lv[first].img_off;
        const long long end = (last < P.nlevels) ? P.lv[last].img_off : P.pix_per_frame;
        ProfScope ps(h, PBD_K_PYRDOWN, st);
        launch_pyrdown_range(pp, nb, first, last, base, end - base, st);
    }
    launch_hog_stage(h, P, cn, depth, f0, nb, st);
}

void launch_hog_stage(pbd_handle *h, Plan &P, int cn, int depth, int f0, int nb, hipStream_t st)
{
    HogParams hp{};
    hp.lv = P.d_lv.p; hp.nlevels = P.nlevels; hp.cn = cn; hp.sbin = h->sbin; hp.frame0 = f0;
    hp.pix_per_frame = P.pix_per_frame; hp.blk_per_frame = P.blk_per_frame; hp.cell_per_frame = P.cell_per_frame;
    hp.pyr = h->pyr.as<uint8_t>(); hp.depth = depth; hp.coord = h->d_coord.p;
    hp.gmag = h->gmag.p; hp.gori = h->gori.as<uint8_t>();
    hp.hist = h->hist.p; hp.norm = h->norm.p; hp.feat = h->feat.p;
    hp.htiles = P.d_htiles.p; hp.nhtiles = P.nhtiles;
    {
        ProfScope ps(h, PBD_K_HOG_HIST, st);
        launch_hog_hist(hp, nb, h->f64, st);
    }
    {
        ProfScope ps(h, PBD_K_HOG_FEAT, st);
        launch_hog_feat(hp, nb, h->f64, st);
    }
}

// the pyramid and HOG features of a mixed plan's virtual frame; d_fd = the call's FrameDesc table (device)
void launch_features_mixed(pbd_handle *h, Plan &P, const FrameDesc *d_fd, int cn, int depth, hipStream_t st)
{
    PyrParams pp{};
    pp.lv = P.d_lv.p; pp.nlevels = P.nlevels; pp.interval = P.interval; pp.cn = cn; pp.frame0 = 0;
    pp.pyr = h->pyr.as<uint8_t>();
    pp.tabx = P.d_tabx.p; pp.taby = P.d_taby.p; pp.depth = depth; pp.tabxf = P.d_tabxf.p; pp.tabyf = P.d_tabyf.p;
    pp.fd = d_fd; pp.lv_frame = P.d_lv_frame.p;
    for (size_t k = 0; k < P.run_n.size(); ++k) {
        pp.run_lev = P.d_run_lev.p + P.run_lev0[k];
        pp.run_off = P.d_run_off.p + P.run_off0[k];
        pp.nruns = P.run_n[k];
        pp.pix_per_frame = P.run_npix[k];   // the launch's pixel count
        if (k == 0) { ProfScope ps(h, PBD_K_RESIZE, st); launch_resize_runs(pp, st); }
        else { ProfScope ps(h, PBD_K_PYRDOWN, st); launch_pyrdown_runs(pp, st); }
    }
    launch_hog_stage(h, P, cn, depth, 0, 1, st);
}

int ensure_seg_tiles(pbd_handle *h, Plan &P, int nb)
{
    if (nb < 1 || P.segtiles.count(nb)) return PBD_OK;
    std::vector<ConvSegTile> tiles;
    build_seg_tiles(P.lv, nb, tiles);
    DevTable<ConvSegTile> t;
    HIPCHK(h, t.upload(tiles));
    P.segtiles[nb] = std::move(t);
    return PBD_OK;
}

int alloc_conv(pbd_handle *h, Plan &P, int nframes)
{
    if (!h->filters_set) return fail(h, PBD_ERR_STATE, "pdf() before setFilters()");
    HIPCHK(h, h->resp.ensure(std::max<size_t>((size_t)nframes * P.cell_per_frame * h->F * h->resp_es, 16) + 32));   // + slack: 16-half chunk reads
    return PBD_OK;
}

void launch_conv_stage(pbd_handle *h, Plan &P, int f0, int nb, hipStream_t st)
{
    ConvParams cp{};
    cp.lv = P.d_lv.p; cp.tiles = P.d_tiles.p; cp.ntiles = P.ntiles;
    cp.shaped = P.d_shaped.p;
    for (int k = 0; k < 3; ++k) cp.nshaped[k] = P.nshaped[k];
    cp.segtiles = nullptr; cp.nsegtiles = 0;
    if (!h->f64 && h->cfg.conv_mode != PBD_CONV_MFMA && h->cfg.conv_mode != PBD_CONV_MFMA_F16) {
        const auto it = P.segtiles.find(nb);     // built by ensure_seg_tiles before the first launch of this many frames
        if (it != P.segtiles.end()) { cp.segtiles = it->second.p; cp.nsegtiles = (int)it->second.size; }
    }
    cp.F = h->F; cp.frame0 = f0;
    cp.cell_per_frame = P.cell_per_frame;
    cp.feat = h->feat.p; cp.resp = h->resp.p;
    cp.fma = h->cfg.conv_mode == PBD_CONV_FMA;
    cp.c31_zero = h->res.c31_zero ? 1 : 0;
    ProfScope ps(h, PBD_K_CONV, st);
    for (const pbd_handle::ConvClass &C : h->conv_classes) {     // one launch per filter size (one class in every known model)
        cp.nf = C.nf; cp.Fpad = C.Fpad; cp.ksize = C.K; cp.wts = C.wts.p; cp.fmap = C.fmap.p;
        const int ngroups = C.Fpad / kConvQ;
        // few workgroups (single frame): split the filter groups over more workgroups to fill the chip
        const long long wgs = (long long)P.ntiles * nb;
        cp.groups_per_block = wgs >= 1024 ? ngroups : std::max(1, (int)(ngroups * wgs / 1024));
        {   // Channels of the haloed tile staged in LDS at a time (generic kernel).  All 32 staged once is the least work, but 110 KB
            // (T = double, 5 x 5) leaves ONE workgroup -- one wave per SIMD -- on a CU and the kernel then waits for its own LDS
            // reads: the largest block within 36 KB (four or more workgroups per CU) is taken, restaged per filter group.
            // Measured, one 640x480 frame, T = double: 9.84 ms with 32 channels -> see profiles/README.md.
            const size_t plane = (size_t)(((kConvTH + C.K - 1) * (kConvTW + C.K - 1)) | 1) * h->rs;
            cp.cblock = 32;
            while (cp.cblock > 1 && cp.cblock * plane > kConvLdsBudget) cp.cblock /= 2;
        }
        cp.wts3 = C.wts3.p;
        cp.unit_f0 = C.unit_f0.p; cp.unit_ql = C.unit_ql.p; cp.unit_woff = C.unit_woff.p; cp.nunits = C.nunits;
        cp.c31tab = C.c31tab.p; cp.c31stride = C.c31stride;
        cp.units_per_block = wgs >= 1024 ? std::max(C.nunits, 1) : std::max(1, (int)((long long)C.nunits * wgs / 1024));
        if (h->cfg.conv_mode == PBD_CONV_MFMA || h->cfg.conv_mode == PBD_CONV_MFMA_F16)
            launch_conv_mfma(cp, h->d_wrec.p, h->cfg.conv_mode == PBD_CONV_MFMA_F16, nb, st);
        else if (h->cfg.conv_mode == PBD_CONV_MFMA_F64) launch_conv_mfma_f64(cp, C.wfrag64.as<double>(), nb, st);
        else launch_conv(cp, nb, h->f64, st);
    }
}

// frames per DP chunk so that the chunk scratch stays within the budget
// DP scratch budget per chunk; a handle's DP_BUDGET_MB debug option lets the tests force several chunks on a small batch
size_t dp_budget(const pbd_handle *h)
{
    return h->dp_budget_mb > 0 ? (size_t)h->dp_budget_mb << 20 : (size_t)8 << 30;
}

// bytes of DP scratch for `cells` cells and `stk` stack records per job (12 B / cell-job + 16 B / two stack entries, float)
size_t dp_scratch_bytes(const pbd_handle *h, long long cells, long long stk)
{
    const size_t JG = (size_t)std::max(h->JGmax, 1);
    return (size_t)cells * JG * (6 + 2 * h->rs) + (size_t)stk * JG * (h->f64 ? kStkPairF64 : kStkPairF32);
}

int dp_chunk_frames(pbd_handle *h, Plan &P, int want)
{
    const size_t per_frame = dp_scratch_bytes(h, P.cell_per_frame, P.stk_per_jf), budget = dp_budget(h);
    int chunk = std::max(want, 1);
    while (chunk > 1 && per_frame * chunk > budget) chunk = (chunk + 1) / 2;
    return chunk;
}

int alloc_dp_scratch(pbd_handle *h, Plan &P, int chunk);

int alloc_dp(pbd_handle *h, Plan &P, int nframes, int chunk)
{
    const size_t cpf = (size_t)P.cell_per_frame;
    const int NSa = std::max(h->NS, 1);
    HIPCHK(h, h->acc.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->NM, 1) * h->rs, 16)));
    const size_t pes = P.ptr8 ? 1 : 2;        // bytes per position
    HIPCHK(h, h->Ik.ensure(std::max<size_t>((size_t)nframes * cpf * NSa, 16)));
    HIPCHK(h, h->rootv.ensure(std::max<size_t>((size_t)nframes * cpf * h->NC * h->rs, 16)));
    HIPCHK(h, h->rooti.ensure(std::max<size_t>((size_t)nframes * cpf * h->NC * sizeof(int), 16)));
    // the transform's pointer planes are kept for the whole batch (one plane per (part, mixture)): the walk composes Ix / Iy from them
    HIPCHK(h, h->IxRaw.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->totmix, 1) * pes, 16) + 32));
    HIPCHK(h, h->IyRaw.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->totmix, 1) * pes, 16) + 32));
    return alloc_dp_scratch(h, P, chunk);
}

// the dynamic program's per-chunk scratch for `chunk` frames of plan P
int alloc_dp_scratch(pbd_handle *h, Plan &P, int chunk)
{
    const size_t cpf = (size_t)P.cell_per_frame;
    const size_t per_frame = cpf * std::max(h->JGmax, 1);
    const size_t stk_per_frame = (size_t)P.stk_per_jf * std::max(h->JGmax, 1);
    HIPCHK(h, h->tmp.ensure(std::max<size_t>(per_frame * chunk * h->rs, 16)));
    HIPCHK(h, h->dt.ensure(std::max<size_t>(per_frame * chunk * h->rs, 16) + 32));            // + slack: the combine step reads whole cell groups
    HIPCHK(h, h->stk.ensure(std::max<size_t>(stk_per_frame * chunk * (h->f64 ? kStkPairF64 : kStkPairF32), 16)));
    return PBD_OK;
}

// dynamic program for frames [f0, f0+nb), nb <= the chunk size given to alloc_dp
// (cell0: a mixed plan's group of whole frames, run as sub-plan P whose cell offsets start at 0 -- the whole-batch buffers are
// addressed from the group's first cell of the virtual frame)
void launch_dp_chunk(pbd_handle *h, Plan &P, int f0, int nb, hipStream_t st, long long cell0 = 0)
{
    DpParams dp{};
    dp.lv = P.d_lv.p; dp.nlevels = P.nlevels; dp.F = h->F; dp.NS = h->NS; dp.NC = h->NC; dp.NM = h->NM;
    dp.cell_per_frame = P.cell_per_frame; dp.quad_per_frame = P.quad_per_frame; dp.max_mix = h->max_mix;
    dp.resp = h->resp.p; dp.resp_half = h->resp_half ? 1 : 0; dp.acc = h->acc.p;
    dp.Ik = h->Ik.as<uint8_t>(); dp.NJ = h->totmix; dp.ptr8 = P.ptr8 ? 1 : 0;
    dp.tmp = h->tmp.p; dp.dt = h->dt.p;
    dp.IxRaw = h->IxRaw.p; dp.IyRaw = h->IyRaw.p;
    dp.stk = h->stk.p; dp.stk_per_jf = P.stk_per_jf;
    dp.stk_row_off = P.d_stk_row_off.p; dp.stk_col_off = P.d_stk_col_off.p;
    dp.biasw = h->d_biasw.p;
    dp.row2level = P.d_row2level.p; dp.rowoff = P.d_rowoff.p; dp.col2level = P.d_col2level.p; dp.coloff = P.d_coloff.p;
    dp.nrows_flat = P.nrows_flat; dp.ncols_flat = P.ncols_flat; dp.longest = P.longest;
    dp.rootv = h->rootv.p; dp.rooti = h->rooti.as<int>(); dp.rjobs = h->d_rjobs.p;
    dp.frame0 = f0;
    if (cell0) {
        const size_t c0 = (size_t)cell0, pes = P.ptr8 ? 1 : 2;
        dp.resp = h->resp.as<char>() + c0 * h->F * h->resp_es;
        dp.acc = h->acc.as<char>() + c0 * h->NM * h->rs;
        dp.Ik = h->Ik.as<uint8_t>() + c0 * h->NS;
        dp.IxRaw = h->IxRaw.as<char>() + c0 * h->totmix * pes;
        dp.IyRaw = h->IyRaw.as<char>() + c0 * h->totmix * pes;
        dp.rootv = h->rootv.as<char>() + c0 * h->NC * h->rs;
        dp.rooti = h->rooti.as<int>() + c0 * h->NC;
    }
    for (auto &g : h->groups) {
        dp.JG = (int)g.jobs.size();
        dp.jobs = g.d_jobs.p; dp.cjobs = g.d_cjobs.p; dp.childs = g.d_childs.p;
        dp.bz_x = g.bz_x; dp.bz_y = g.bz_y;
        { ProfScope ps(h, PBD_K_DT_ROWS, st); launch_dt_rows(dp, h->dt_opt, nb, h->f64, st); }
        { ProfScope ps(h, PBD_K_DT_COLS, st); launch_dt_cols(dp, h->dt_opt, nb, h->f64, st); }
        dp.sjobs = g.d_sjobs.p;
        {
            ProfScope ps(h, PBD_K_DP_COMBINE, st);
            if (h->seq_mode) launch_dp_combine_seq(dp, (int)g.sjobs.size(), nb, h->f64, st);
            else launch_dp_combine(dp, (int)g.cjobs.size(), nb, h->f64, st);
        }
    }
    { ProfScope ps(h, PBD_K_DP_ROOT, st); launch_dp_root(dp, nb, h->f64, st); }
}

// the stages over the whole batch on the handle's stream (the dynamic program in chunks of frames within its scratch budget)
int run_conv(pbd_handle *h, Plan &P, int nframes)
{
    if (int rc = alloc_conv(h, P, nframes)) return rc;
    if (int rc = ensure_seg_tiles(h, P, nframes)) return rc;
    launch_conv_stage(h, P, 0, nframes, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.resp = true;
    return PBD_OK;
}

int run_dp(pbd_handle *h, Plan &P, int nframes)
{
    const int chunk = dp_chunk_frames(h, P, nframes);
    if (int rc = alloc_dp(h, P, nframes, chunk)) return rc;
    for (int f0 = 0; f0 < nframes; f0 += chunk) launch_dp_chunk(h, P, f0, std::min(chunk, nframes - f0), h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.dp = true;
    return PBD_OK;
}

// ---- argmin: find (ordered compaction) + walk into a device payload, then one D2H ---------------------------------
// enqueues the find and walk kernels for the `nframes` frames of the device-resident DP result; the candidate list is
// written to d_payload = int32[1 + capacity * stride] (see pbd_handle::CandBuf).  No host synchronisation.
int enqueue_argmin(pbd_handle *h, Plan &P, int nframes, const float *d_scales, int frame_offset, int32_t *d_payload,
                   int capacity, hipStream_t st, bool walk_only = false)
{
    ArgminParams ap{};
    ap.lv = P.d_lv.p; ap.nlevels = P.nlevels; ap.NS = h->NS; ap.NC = h->NC; ap.nframes = nframes;
    ap.cell_per_frame = P.cell_per_frame;
    ap.rootv = h->rootv.p; ap.rooti = h->rooti.as<int>();
    ap.IxRaw = h->IxRaw.p; ap.IyRaw = h->IyRaw.p; ap.NJ = h->totmix; ap.Ik = h->Ik.as<uint8_t>(); ap.ptr8 = P.ptr8 ? 1 : 0;
    ap.thresh = h->thresh; ap.scales = d_scales;
    ap.walk = h->d_walk.p; ap.walk_off = h->d_walk_off.p;
    ap.max_parts = h->max_parts; ap.stride = stride(h); ap.capacity = std::max(capacity, 0);
    ap.payload = d_payload; ap.frame_offset = frame_offset;
    if (P.kind == 2) { ap.lv_frame = P.d_lv_frame.p; ap.lv_local = P.d_lv_local.p; }
    ap.ntotal = (long long)nframes * P.cell_per_frame * h->NC;
    ap.nblk = (int)std::max<long long>((ap.ntotal + argmin_find_span() - 1) / argmin_find_span(), 1);
    HIPCHK(h, h->find_blk.ensure((size_t)ap.nblk * sizeof(int)));
    ap.blk = h->find_blk.as<int>();
    ProfScope ps(h, PBD_K_ARGMIN, st);
    if (!walk_only) launch_argmin_find(ap, h->f64, st);   // walk_only: the payload's records were written by the caller
    launch_argmin_walk(ap, h->f64, st);
    return PBD_OK;
}

// ---- post-processing (pbd_set_nms): per-frame sort + suppression of the payload d_in (capacity in_cap records, frame-local
// `frame` fields, nframes frames of rows x cols) into d_out = int32[1 + out_cap * stride]: word 0 = kept count (-1 when more
// than in_cap candidates were found), then the kept records frame by frame, `frame` + frame_offset.  No host synchronisation.
// pbd_suppress*: `in_offset` is subtracted from the input's `frame` fields and `bad` (zeroed here) turns on the list's check.
int enqueue_post(pbd_handle *h, int nframes, int rows, int cols, float overlap, const int32_t *d_in, int in_cap, int frame_offset,
                 int32_t *d_out, int out_cap, hipStream_t st, const Plan *mixed = nullptr, int in_offset = 0, int *bad = nullptr)
{
    PostParams pp{};
    pp.in_offset = in_offset; pp.bad = bad;
    if (bad) HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), st));
    pp.in = d_in; pp.in_cap = std::max(in_cap, 1);
    pp.stride = stride(h); pp.max_parts = h->max_parts; pp.nframes = nframes;
    pp.rows = rows; pp.cols = cols; pp.wpr = (cols + 31) / 32; pp.overlap = overlap;
    pp.out = d_out; pp.out_cap = std::max(out_cap, 0); pp.frame_offset = frame_offset;
    // workspace: key, frame, perm, slot [in_cap] | box [in_cap] int4 | fkept [nframes] | global canvases (frames too big for LDS)
    const size_t n = (size_t)pp.in_cap, a4 = (4 * n * sizeof(int) + 15) & ~(size_t)15;
    const size_t fk = ((size_t)nframes * sizeof(int) + 15) & ~(size_t)15;
    const size_t canvas = mixed ? mixed->post_glb_words * sizeof(uint32_t)
                                : post_canvas_in_lds(rows, cols) ? 0 : (size_t)nframes * post_canvas_words(rows, cols) * sizeof(uint32_t);
    HIPCHK(h, h->post_ws.ensure(a4 + n * sizeof(int4) + fk + canvas));
    char *ws = h->post_ws.as<char>();
    pp.key = reinterpret_cast<float *>(ws); pp.frame = reinterpret_cast<int *>(ws) + n;
    pp.perm = reinterpret_cast<int *>(ws) + 2 * n; pp.slot = reinterpret_cast<int *>(ws) + 3 * n;
    pp.box = reinterpret_cast<int4 *>(ws + a4);
    pp.fkept = reinterpret_cast<int *>(ws + a4 + n * sizeof(int4));
    pp.canvas = canvas ? reinterpret_cast<uint32_t *>(ws + a4 + n * sizeof(int4) + fk) : nullptr;
    if (mixed) {   // every frame with its own size and canvas kind
        pp.fdim = mixed->d_fdim.p; pp.fcanvas = mixed->d_fcanvas.p;
        launch_postprocess_mixed(pp, mixed->d_post_lds.p, (int)mixed->post_lds.size(), mixed->post_lds_words, mixed->d_post_glb.p,
                                 (int)mixed->post_glb.size(), st);
        return PBD_OK;
    }
    launch_postprocess(pp, st);
    return PBD_OK;
}

// find + walk into cb.payload (then, with `post`, the sort + suppression into cb.post) and the speculative read-back of
// [count | first records], all on `st`
int enqueue_argmin_readback(pbd_handle *h, Plan &P, int nframes, const float *d_scales, pbd_handle::CandBuf &cb, bool post,
                            hipStream_t st)
{
    const int stride = ::stride(h), cap = std::max(h->cfg.max_candidates, 1);
    HIPCHK(h, cb.payload.ensure(((size_t)cap * stride + 1) * sizeof(int32_t)));
    if (int rc = enqueue_argmin(h, P, nframes, d_scales, 0, cb.payload.as<int32_t>(), cap, st)) return rc;
    cb.nms = post;
    if (post) {
        HIPCHK(h, cb.post.ensure(((size_t)cap * stride + 1) * sizeof(int32_t)));
        if (int rc = enqueue_post(h, P.kind == 2 ? P.mixed_frames : nframes, P.rows, P.cols, h->nms_overlap, cb.payload.as<int32_t>(),
                                  cap, 0, cb.post.as<int32_t>(), cap, st, P.kind == 2 ? &P : nullptr))
            return rc;
    }
    cb.copied = std::min(h->cand_guess, cap);
    const size_t words = 1 + (size_t)cb.copied * stride;
    // the mirror is sized for twice the guess: growing pinned memory synchronises the device
    if (cb.host.size < words * sizeof(int32_t))
        HIPCHK(h, cb.reserve(1 + (size_t)std::min(2 * (long long)cb.copied, (long long)cap) * stride));
    HIPCHK(h, hipMemcpyAsync(cb.words(), cb.out().p, words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return PBD_OK;
}

// after the read-back has completed: hand the records to the caller (the reference's order is nondeterministic,
// src/DynamicProgram.cpp:246-251; here it is (frame, level, component, y, x), produced on the device)
int argmin_deliver(pbd_handle *h, pbd_handle::CandBuf &cb, hipStream_t st, int32_t *cand, int capacity, int *ncand)
{
    const int stride = ::stride(h), cap = std::max(h->cfg.max_candidates, 1);
    const int found = cb.words()[0];
    if (found < 0) {         // the post-processing stage saw more candidates than the list holds: no suppressed prefix
        *ncand = 0;
        return fail(h, PBD_ERR_CAPACITY, "more than max_candidates (%d) candidates were found before non-maxima suppression: "
                    "raise pbd_config.max_candidates", cap);
    }
    const int n = std::min(found, cap);
    if (n > cb.copied) {     // more candidates than the speculative copy covered: fetch the list again, whole
        const size_t words = 1 + (size_t)n * stride;
        HIPCHK(h, cb.reserve(words));
        HIPCHK(h, hipMemcpyAsync(cb.words(), cb.out().p, words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        cb.copied = n;
    }
    h->cand_guess = std::min(cap, std::max(n + n / 4 + 256, 1024));
    const int nout = std::min(n, std::max(capacity, 0));
    if (nout > 0) memcpy(cand, cb.words() + 1, (size_t)nout * stride * sizeof(int32_t));
    *ncand = nout;
    if (found > cap || n > capacity)
        return fail(h, PBD_ERR_CAPACITY, "%d candidates found, capacity %d (config max_candidates %d)", found, capacity, cap);
    return PBD_OK;
}

int run_argmin(pbd_handle *h, Plan &P, int nframes, const float *d_scales, bool post, int32_t *cand, int capacity, int *ncand)
{
    if (int rc = enqueue_argmin_readback(h, P, nframes, d_scales, h->cb, post, h->stream)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return argmin_deliver(h, h->cb, h->stream, cand, capacity, ncand);
}

// the device-out form: the list straight into the caller's payload, or -- with the post-processing stage on -- the whole list
// into the handle's own payload (capacity max_candidates: the stage never sees a truncated list), then the kept records into
// the caller's
int enqueue_argmin_out(pbd_handle *h, Plan &P, int nframes, int frame_offset, int32_t *d_payload, int capacity)
{
    if (!h->nms) return enqueue_argmin(h, P, nframes, P.d_scales.p, frame_offset, d_payload, capacity, h->stream);
    const int cap = std::max(h->cfg.max_candidates, 1);
    HIPCHK(h, h->cb.payload.ensure(((size_t)cap * stride(h) + 1) * sizeof(int32_t)));
    if (int rc = enqueue_argmin(h, P, nframes, P.d_scales.p, 0, h->cb.payload.as<int32_t>(), cap, h->stream)) return rc;
    return enqueue_post(h, P.kind == 2 ? P.mixed_frames : nframes, P.rows, P.cols, h->nms_overlap, h->cb.payload.as<int32_t>(), cap,
                        frame_offset, d_payload, capacity, h->stream, P.kind == 2 ? &P : nullptr);
}

// Frames of a call: on the host (`host[i]`, rows `stride` bytes apart; uploaded to h->frames by enqueue_features) or
// already packed on the device (`dev`)
struct FrameSrc {
    const void *const *host;
    size_t stride;
    const void *dev;
};

// image depth and channels; for host frames also the row stride and, for 32F / 64F, that every pixel is finite
int check_frames(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth)
{
    if (!depth_size(depth))
        return fail(h, PBD_ERR_UNSUPPORTED, "image depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F), src/HOGFeatures.cpp:136-146", depth);
    if (cn != 1 && cn != 3) return fail(h, PBD_ERR_INVALID, "channels %d (1 or 3, src/HOGFeatures.cpp:171)", cn);
    if (!src.host) return PBD_OK;
    const size_t row_bytes = (size_t)cols * cn * depth_size(depth);
    if (src.stride < row_bytes) return fail(h, PBD_ERR_INVALID, "stride %zu < row bytes %zu", src.stride, row_bytes);
    // 32F / 64F images: a NaN or Inf pixel is refused.  The reference computes *something* deterministic from one (NaN
    // gradients, NaN histogram bins, NaN responses whose envelope read-out order then matters); the distance transform here
    // walks the envelope top-down, which equals the reference's bottom-up walk only for strictly increasing finite
    // intersections -- so non-finite input is defined as an error instead of being allowed to differ silently.
    if (depth == kDepth32F || depth == kDepth64F) {
        const size_t n = (size_t)cols * cn;
        for (int i = 0; i < nframes; ++i)
            for (int y = 0; y < rows; ++y) {
                const char *row = static_cast<const char *>(src.host[i]) + (size_t)y * src.stride;
                bool ok = true;
                if (depth == kDepth32F) { const float *p = reinterpret_cast<const float *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(p[k]); }
                else { const double *p = reinterpret_cast<const double *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(p[k]); }
                if (!ok) return fail(h, PBD_ERR_INVALID, "frame %d, row %d holds a NaN or Inf pixel", i, y);
            }
    }
    return PBD_OK;
}

// every check of a detect call, before anything is enqueued; *plan = the batch's image plan
int check_detect(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth, Plan **plan)
{
    if (int rc = check_batch(h, nframes)) return rc;
    if (int rc = check_frames(h, nframes, src, rows, cols, cn, depth)) return rc;
    if (int rc = check_bank(h)) return rc;
    return get_image_plan(h, rows, cols, plan);
}

int upload_frames(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int cn, int depth, size_t stride_bytes)
{
    const size_t row_bytes = (size_t)cols * cn * depth_size(depth);
    HIPCHK(h, h->frames.ensure((size_t)nframes * rows * row_bytes + 4));
    for (int i = 0; i < nframes; ++i)
        HIPCHK(h, hipMemcpy2DAsync(h->frames.as<uint8_t>() + (size_t)i * rows * row_bytes, row_bytes, imgs[i], stride_bytes,
                                   row_bytes, rows, hipMemcpyHostToDevice, h->stream));
    return PBD_OK;
}

// The batch's result replaces the resident one here; then its frames are uploaded (host frames) and the pyramid and HOG
// features enqueued.  No host synchronisation.
int enqueue_features(pbd_handle *h, Plan &P, int nframes, const FrameSrc &src, int cn, int depth)
{
    h->res = Resident{&P, nframes, cn, depth};
    const void *d_frames = src.dev;
    if (src.host) {
        if (int rc = upload_frames(h, nframes, src.host, P.rows, P.cols, cn, depth, src.stride)) return rc;
        d_frames = h->frames.p;
    }
    if (int rc = alloc_features(h, P, nframes, cn, depth)) return rc;
    launch_features(h, P, d_frames, cn, depth, 0, nframes, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.features = h->res.c31_zero = true;
    return PBD_OK;
}

// pyramid -> HOG -> convolution -> dynamic program for a batch that passed check_detect (no host synchronisation)
int enqueue_detect(pbd_handle *h, Plan &P, int nframes, const FrameSrc &src, int cn, int depth)
{
    if (int rc = enqueue_features(h, P, nframes, src, cn, depth)) return rc;
    if (int rc = run_conv(h, P, nframes)) return rc;
    return run_dp(h, P, nframes);
}

// the synchronous detect entry points: the whole path, then the candidates' read-back
int detect_sync(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth, int32_t *cand, int capacity,
                int *ncand)
{
    Plan *P = nullptr;
    if (int rc = check_detect(h, nframes, src, rows, cols, cn, depth, &P)) return rc;
    if (int rc = enqueue_detect(h, *P, nframes, src, cn, depth)) return rc;
    return run_argmin(h, *P, nframes, P->d_scales.p, h->nms, cand, capacity, ncand);
}

// copies n responses from the device to dst as T; in PBD_CONV_MFMA_F16 mode the device holds fp16, widened to float here
int read_responses(pbd_handle *h, void *dst, const void *src, size_t n)
{
    if (!n) return PBD_OK;
    if (!h->resp_half) {
        HIPCHK(h, hipMemcpyAsync(dst, src, n * h->rs, hipMemcpyDeviceToHost, h->stream));
        return PBD_OK;
    }
    std::vector<uint16_t> halfbuf(n);
    HIPCHK(h, hipMemcpyAsync(halfbuf.data(), src, n * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float *out = static_cast<float *>(dst);
    for (size_t i = 0; i < n; ++i) out[i] = host_h2f(halfbuf[i]);
    return PBD_OK;
}

// ---- mixed-size calls (pbd_detect_frames*) -------------------------------------------------------------------------------
// the dynamic program of a mixed plan: the whole virtual frame in one pass when its scratch fits the budget, else in groups
// of whole frames (sub-plans built once per budget)
int run_dp_mixed(pbd_handle *h, Plan &P)
{
    const size_t budget = dp_budget(h);
    auto scratch = [&](long long cells, long long stk) { return dp_scratch_bytes(h, cells, stk); };
    if (int rc = alloc_dp(h, P, 1, 0)) return rc;   // the whole-batch buffers (scratch below)
    if (scratch(P.cell_per_frame, P.stk_per_jf) <= budget || P.mixed_frames == 1) {
        if (int rc = alloc_dp_scratch(h, P, 1)) return rc;
        launch_dp_chunk(h, P, 0, 1, h->stream);
    } else {
        if (P.chunk_budget != budget) {
            // groups of consecutive frames, greedily, by an estimate (cells, and the stack share of the virtual frame's)
            std::vector<std::unique_ptr<Plan>> plans;
            std::vector<long long> cell0s;
            int f = 0;
            while (f < P.mixed_frames) {
                int g = f + 1;
                auto cells = [&](int a, int b) {
                    const int l0 = P.frame_lv0[a], l1 = P.frame_lv0[b];
                    return (l1 < P.nlevels ? P.lv[l1].cell_off : P.cell_per_frame) - P.lv[l0].cell_off;
                };
                auto est = [&](int a, int b) {
                    const long long c = cells(a, b);
                    return scratch(c, P.cell_per_frame ? (long long)((double)P.stk_per_jf * c / P.cell_per_frame) + 64 : 0);
                };
                while (g < P.mixed_frames && est(f, g + 1) <= budget) ++g;
                auto S = std::make_unique<Plan>();
                const int l0 = P.frame_lv0[f], l1 = P.frame_lv0[g];
                const long long c0 = P.lv[l0].cell_off;
                S->kind = 3; S->interval = P.interval; S->nlevels = l1 - l0;
                S->lv.assign(P.lv.begin() + l0, P.lv.begin() + l1);
                for (LevelDesc &d : S->lv) d.cell_off -= c0;
                S->cell_per_frame = cells(f, g);
                HIPCHK(h, finish_plan_tables(*S, h->sbin));
                S->ptr8 = P.ptr8;        // the pointer planes' element size is the whole call's
                plans.push_back(std::move(S));
                cell0s.push_back(c0);
                f = g;
            }
            P.chunk_plans = std::move(plans);
            P.chunk_cell0 = std::move(cell0s);
            P.chunk_budget = budget;
        }
        for (auto &S : P.chunk_plans)
            if (int rc = alloc_dp_scratch(h, *S, 1)) return rc;
        for (size_t i = 0; i < P.chunk_plans.size(); ++i) launch_dp_chunk(h, *P.chunk_plans[i], 0, 1, h->stream, P.chunk_cell0[i]);
    }
    HIPCHK(h, hipGetLastError());
    h->res.dp = true;
    return PBD_OK;
}

// every check of a mixed-size call before anything is enqueued; *plan = its mixed plan
int check_frames_mixed(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host, Plan **plan)
{
    if (h->shard_world > 1)
        return fail(h, PBD_ERR_UNSUPPORTED, "mixed-size calls with level sharding (world %d): pbd_set_level_shard(h, 0, 1) first",
                    h->shard_world);
    if (int rc = check_batch(h, nframes)) return rc;
    if (!depth_size(depth))
        return fail(h, PBD_ERR_UNSUPPORTED, "image depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F), src/HOGFeatures.cpp:136-146", depth);
    if (cn != 1 && cn != 3) return fail(h, PBD_ERR_INVALID, "channels %d (1 or 3, src/HOGFeatures.cpp:171)", cn);
    std::vector<int> rows(nframes), cols(nframes);
    for (int f = 0; f < nframes; ++f) {
        const pbd_frame &fr = frames[f];
        if (!fr.data || fr.rows < 1 || fr.cols < 1 || fr.rows > 32000 || fr.cols > 32000)
            return fail(h, PBD_ERR_INVALID, "frame %d: %dx%d at %p", f, fr.rows, fr.cols, fr.data);
        const size_t row_bytes = (size_t)fr.cols * cn * depth_size(depth);
        if (fr.stride_bytes < row_bytes) return fail(h, PBD_ERR_INVALID, "frame %d: stride %zu < row bytes %zu", f, fr.stride_bytes, row_bytes);
        if (!host && (reinterpret_cast<uintptr_t>(fr.data) % depth_size(depth) || fr.stride_bytes % depth_size(depth)))
            return fail(h, PBD_ERR_INVALID, "frame %d: device pointer %p / stride %zu not a multiple of the %zu-byte element", f, fr.data,
                        fr.stride_bytes, depth_size(depth));
        if (host && (depth == kDepth32F || depth == kDepth64F)) {   // as check_frames: non-finite input is an error
            const size_t n = (size_t)fr.cols * cn;
            for (int y = 0; y < fr.rows; ++y) {
                const char *row = static_cast<const char *>(fr.data) + (size_t)y * fr.stride_bytes;
                bool ok = true;
                if (depth == kDepth32F) { const float *q = reinterpret_cast<const float *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(q[k]); }
                else { const double *q = reinterpret_cast<const double *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(q[k]); }
                if (!ok) return fail(h, PBD_ERR_INVALID, "frame %d, row %d holds a NaN or Inf pixel", f, y);
            }
        }
        rows[f] = fr.rows; cols[f] = fr.cols;
    }
    if (int rc = check_bank(h)) return rc;
    return get_mixed_plan(h, nframes, rows.data(), cols.data(), plan);
}

// pyramid -> HOG -> convolution -> dynamic program of a mixed-size call that passed check_frames_mixed (no host synchronisation)
int enqueue_detect_mixed(pbd_handle *h, Plan &P, int nframes, const pbd_frame *frames, int cn, int depth, bool host,
                         const LatentParams *mask = nullptr)
{
    h->res = Resident{&P, 1, cn, depth};
    const size_t es = depth_size(depth);
    std::vector<FrameDesc> fd(nframes);
    if (host) {   // the frames go to the handle's frame buffer, packed, each with its own dense rows
        size_t total = 0;
        for (int f = 0; f < nframes; ++f) total += (size_t)frames[f].rows * frames[f].cols * cn * es;
        HIPCHK(h, h->frames.ensure(total + 4));
        size_t off = 0;
        for (int f = 0; f < nframes; ++f) {
            const size_t row_bytes = (size_t)frames[f].cols * cn * es;
            uint8_t *dst = h->frames.as<uint8_t>() + off;
            HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, frames[f].data, frames[f].stride_bytes, row_bytes, frames[f].rows,
                                       hipMemcpyHostToDevice, h->stream));
            fd[f] = FrameDesc{dst, frames[f].rows, frames[f].cols, (long long)row_bytes};
            off += row_bytes * frames[f].rows;
        }
    } else {
        for (int f = 0; f < nframes; ++f)
            fd[f] = FrameDesc{static_cast<const uint8_t *>(frames[f].data), frames[f].rows, frames[f].cols, (long long)frames[f].stride_bytes};
    }
    const size_t fd_bytes = fd.size() * sizeof(FrameDesc);
    if (h->fd_copied.p) HIPCHK(h, hipEventSynchronize(h->fd_copied.p));   // the previous call's table has left the staging buffer
    else HIPCHK(h, hipEventCreateWithFlags(&h->fd_copied.p, hipEventDisableTiming));
    HIPCHK(h, h->fd_host.ensure(fd_bytes, fd_bytes * 2 + 256));
    HIPCHK(h, h->fd_dev.ensure(fd_bytes));
    memcpy(h->fd_host.p, fd.data(), fd_bytes);
    HIPCHK(h, hipMemcpyAsync(h->fd_dev.p, h->fd_host.p, fd_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->fd_copied.p, h->stream));
    if (int rc = alloc_features(h, P, 1, cn, depth)) return rc;
    launch_features_mixed(h, P, h->fd_dev.as<FrameDesc>(), cn, depth, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.features = h->res.c31_zero = true;
    if (int rc = run_conv(h, P, 1)) return rc;
    if (mask) {   // pbd_detect_latent: the responses of the latent bank, masked before the dynamic program
        LatentParams lp = *mask;
        lp.resp = h->resp.p; lp.lv = P.d_lv.p; lp.nlevels = P.nlevels; lp.F = h->F; lp.cell_per_frame = P.cell_per_frame;
        lp.lv_frame = P.d_lv_frame.p; lp.scales = P.d_scales.p;
        launch_latent_mask(lp, h->f64, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    return run_dp_mixed(h, P);
}

// ---- 3-D boxes from a depth image (pbd_boxes3d*; pbd_kernels_depth.hip)
// the derivative-of-Gaussian taps of Candidate::boundingBox3D (include/Candidate.hpp:190-193), once, with the C library's exp:
//   g = getGaussianKernel(35, 4, CV_32F): t_i = exp(scale2X * x_i * x_i), x_i = i - 17, scale2X = -0.5 / 16; cf_i = (float)t_i,
//       sum += cf_i in double, then cf_i = (float)(cf_i * (1. / sum))
//   dog = filter2D(g, -1, [-1 0 1]^T): correlation, BORDER_REFLECT_101, s = 0; s += k * x per non-zero tap, in float
const float *boxes3d_taps()
{
    static const struct Taps {
        float v[kB3Taps];
        Taps()
        {
            float g[kB3Taps];
            const double scale2X = -0.5 / (4.0 * 4.0);
            double sum = 0;
            for (int i = 0; i < kB3Taps; ++i) {
                const double x = i - (kB3Taps - 1) * 0.5;
                g[i] = (float)exp(scale2X * x * x);
                sum += g[i];
            }
            sum = 1. / sum;
            for (int i = 0; i < kB3Taps; ++i) g[i] = (float)(g[i] * sum);
            for (int i = 0; i < kB3Taps; ++i) {
                const int a = i == 0 ? 1 : i - 1, b = i == kB3Taps - 1 ? kB3Taps - 2 : i + 1;
                float s = 0.f;
                s = s + -1.f * g[a];
                s = s + 1.f * g[b];
                v[i] = s;
            }
        }
    } taps;
    return taps.v;
}

// every check of a pbd_boxes3d* call's frames before anything is enqueued
int check_boxes3d_frames(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                         bool host)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (!depth_size(depth_code))
        return fail(h, PBD_ERR_INVALID, "depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F)", depth_code);
    const size_t es = depth_size(depth_code);
    for (int f = 0; f < nframes; ++f) {
        const pbd_frame &d = depth[f];
        if (!d.data || d.rows < 1 || d.cols < 1 || im_rows[f] < 1 || im_cols[f] < 1)
            return fail(h, PBD_ERR_INVALID, "frame %d: depth %dx%d at %p, colour frame %dx%d", f, d.rows, d.cols, d.data, im_rows[f],
                        im_cols[f]);
        // every box lies inside the depth image: the samples of one record (boxes counted with their overlaps) fit an int
        if ((unsigned long long)kB3MaxBoxes * (unsigned long long)d.rows * (unsigned long long)d.cols >= (1ull << 31))
            return fail(h, PBD_ERR_INVALID, "frame %d: depth image %dx%d too large", f, d.rows, d.cols);
        if (d.stride_bytes < (size_t)d.cols * es)
            return fail(h, PBD_ERR_INVALID, "frame %d: stride %zu < row bytes %zu", f, d.stride_bytes, (size_t)d.cols * es);
        if (!host && (reinterpret_cast<uintptr_t>(d.data) % es || d.stride_bytes % es))
            return fail(h, PBD_ERR_INVALID, "frame %d: device pointer %p / stride %zu not a multiple of the %zu-byte element", f, d.data,
                        d.stride_bytes, es);
    }
    return PBD_OK;
}

// the frame table to the device (through the pinned staging buffer) and the kernel, on the handle's stream
int enqueue_boxes3d(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, const int32_t *d_payload, int capacity,
                    int frame_offset, double *d_out)
{
    const size_t bytes = tab.size() * sizeof(Box3dFrame);
    if (h->b3_tab_copied.p) HIPCHK(h, hipEventSynchronize(h->b3_tab_copied.p));   // the previous call's table has left the staging buffer
    else HIPCHK(h, hipEventCreateWithFlags(&h->b3_tab_copied.p, hipEventDisableTiming));
    HIPCHK(h, h->b3_tab_host.ensure(bytes, bytes * 2 + 256));
    HIPCHK(h, h->b3_tab.ensure(bytes));
    memcpy(h->b3_tab_host.p, tab.data(), bytes);
    HIPCHK(h, hipMemcpyAsync(h->b3_tab.p, h->b3_tab_host.p, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->b3_tab_copied.p, h->stream));
    Boxes3dParams bp{};
    bp.in = d_payload; bp.in_cap = capacity;
    bp.stride = stride(h); bp.max_parts = h->max_parts;
    bp.frames = h->b3_tab.as<Box3dFrame>(); bp.nframes = (int)tab.size(); bp.frame_offset = frame_offset;
    bp.depth = depth_code; bp.out = d_out;
    memcpy(bp.dog, boxes3d_taps(), sizeof bp.dog);
    launch_boxes3d(bp, capacity, h->stream);
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the host records of a pbd_boxes3d* call: frame index and part count of each
int check_boxes3d_records(pbd_handle *h, int nframes, const int32_t *cand, int ncand, int frame_offset)
{
    const int stride = ::stride(h);
    for (int i = 0; i < ncand; ++i) {
        const int32_t *r = cand + (size_t)i * stride;
        const long long f = (long long)r[0] - frame_offset;
        if (f < 0 || f >= nframes)
            return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d outside 0..%d", i, r[0], frame_offset, nframes - 1);
        if (r[6] < 1 || r[6] > h->max_parts) return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (1..%d)", i, r[6], h->max_parts);
    }
    return PBD_OK;
}

// the host forms' depth images (packed with dense rows) and records (as a payload) into the handle's own buffers
int upload_boxes3d_host(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                        const int32_t *cand, int ncand, std::vector<Box3dFrame> &tab)
{
    const int stride = ::stride(h);
    const size_t es = depth_size(depth_code);
    size_t total = 0;
    for (int f = 0; f < nframes; ++f) total += (size_t)depth[f].rows * depth[f].cols * es;
    HIPCHK(h, h->b3_depth.ensure(total + 8));
    HIPCHK(h, h->b3_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    tab.resize(nframes);
    size_t off = 0;
    for (int f = 0; f < nframes; ++f) {
        const size_t row_bytes = (size_t)depth[f].cols * es;
        uint8_t *dst = h->b3_depth.as<uint8_t>() + off;
        HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, depth[f].data, depth[f].stride_bytes, row_bytes, depth[f].rows,
                                   hipMemcpyHostToDevice, h->stream));
        tab[f] = Box3dFrame{dst, depth[f].rows, depth[f].cols, (long long)row_bytes, im_rows[f], im_cols[f]};
        off += row_bytes * depth[f].rows;
    }
    HIPCHK(h, hipMemcpyAsync(h->b3_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->b3_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                             h->stream));
    return PBD_OK;
}

// a small table to the device through pinned staging memory, which is rewritten only once its previous copy has completed
int stage_table(pbd_handle *h, HostBuf &host, DevBuf &dev, Event &copied, const void *src, size_t bytes)
{
    if (copied.p) HIPCHK(h, hipEventSynchronize(copied.p));
    else HIPCHK(h, hipEventCreateWithFlags(&copied.p, hipEventDisableTiming));
    HIPCHK(h, host.ensure(bytes, bytes * 2 + 256));
    HIPCHK(h, dev.ensure(bytes));
    memcpy(host.p, src, bytes);
    HIPCHK(h, hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(copied.p, h->stream));
    return PBD_OK;
}

// ---- depth consistency (pbd_depth_consistency*; pbd_kernels_consistency.hip)
// the model's tables the decision reads, uploaded on first use: part offsets, component-local parents, and per part the norm of
// its mixture-0 anchor, std::sqrt((double)ax*ax + (double)ay*ay) (part.anchor(0): src/SearchSpacePruning.cpp:83)
int dc_model_tables(pbd_handle *h)
{
    if (h->dc_norm.p) return PBD_OK;
    const int totparts = (int)h->parentid.size();
    std::vector<double> norm(std::max(totparts, 1), 0.0);
    for (int c = 0; c < h->NC; ++c)
        for (int gp = h->part_offset[c] + 1; gp < h->part_offset[c + 1]; ++gp) {
            const int d = h->defid[h->mix_offset[gp]];
            if (d < 0 || 2 * (size_t)d + 1 >= h->anchors.size()) continue;
            const double ax = h->anchors[2 * (size_t)d], ay = h->anchors[2 * (size_t)d + 1];
            norm[gp] = std::sqrt(ax * ax + ay * ay);
        }
    HIPCHK(h, h->dc_part_offset.upload(h->part_offset));
    HIPCHK(h, h->dc_parent.upload(h->parentid));
    HIPCHK(h, h->dc_norm.upload(norm));
    return PBD_OK;
}

// every check of a pbd_depth_consistency* call's images and zfactor before anything is enqueued
int check_dc_frames(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, float zfactor, bool host)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (!depth_size(depth_code))
        return fail(h, PBD_ERR_INVALID, "depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F)", depth_code);
    if (std::isnan(zfactor)) return fail(h, PBD_ERR_INVALID, "zfactor is NaN");
    const size_t es = depth_size(depth_code);
    for (int f = 0; f < nframes; ++f) {
        const pbd_frame &d = depth[f];
        if (!d.data || d.rows < 1 || d.cols < 1) return fail(h, PBD_ERR_INVALID, "frame %d: depth %dx%d at %p", f, d.rows, d.cols, d.data);
        if ((long long)d.rows * d.cols >= (1LL << 31)) return fail(h, PBD_ERR_INVALID, "frame %d: depth image %dx%d too large", f, d.rows, d.cols);
        if (d.stride_bytes < (size_t)d.cols * es)
            return fail(h, PBD_ERR_INVALID, "frame %d: stride %zu < row bytes %zu", f, d.stride_bytes, (size_t)d.cols * es);
        if (!host && (reinterpret_cast<uintptr_t>(d.data) % es || d.stride_bytes % es))
            return fail(h, PBD_ERR_INVALID, "frame %d: device pointer %p / stride %zu not a multiple of the %zu-byte element", f, d.data,
                        d.stride_bytes, es);
    }
    return PBD_OK;
}

// the host form's records: frame index, component and part count of each
int check_dc_records(pbd_handle *h, int nframes, const int32_t *cand, int ncand, int frame_offset)
{
    const int stride = ::stride(h);
    for (int i = 0; i < ncand; ++i) {
        const int32_t *r = cand + (size_t)i * stride;
        const long long f = (long long)r[0] - frame_offset;
        if (f < 0 || f >= nframes)
            return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d outside 0..%d", i, r[0], frame_offset, nframes - 1);
        if (r[1] < 0 || r[1] >= h->NC) return fail(h, PBD_ERR_INVALID, "record %d: component %d (0..%d)", i, r[1], h->NC - 1);
        const int np = h->part_offset[r[1] + 1] - h->part_offset[r[1]];
        if (r[6] != np || r[6] < 1 || r[6] > h->max_parts)
            return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (component %d has %d)", i, r[6], r[1], np);
    }
    return PBD_OK;
}

// the frame table and the filter's kernels on the handle's stream: payload d_in (capacity records) -> d_out (out_cap records)
int enqueue_dc(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, float zfactor, const int32_t *d_in, int capacity,
               int frame_offset, int32_t *d_out, int out_cap)
{
    if (int rc = dc_model_tables(h)) return rc;
    const int cap = std::max(capacity, 0);
    const long long tasks = std::max<long long>((long long)cap * h->max_parts, 1);
    if (tasks >= (1LL << 30)) return fail(h, PBD_ERR_INVALID, "capacity %d: %lld parts (below 2^30)", capacity, tasks);
    const int blocks = dc_record_blocks(cap);
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t s_med = al(tasks * sizeof(double)), s_queue = al(tasks * sizeof(int)), s_qn = 256,
                 s_flag = al((size_t)blocks * 256 * sizeof(int)), s_blk = al((size_t)blocks * sizeof(int));
    HIPCHK(h, h->dc_ws.ensure(s_med + s_queue + s_qn + s_flag + s_blk));
    if (int rc = stage_table(h, h->dc_tab_host, h->dc_tab, h->dc_tab_copied, tab.data(), tab.size() * sizeof(Box3dFrame))) return rc;
    uint8_t *w = h->dc_ws.as<uint8_t>();
    DcParams p{};
    p.in = d_in; p.in_cap = cap; p.stride = stride(h); p.max_parts = h->max_parts;
    p.frames = h->dc_tab.as<Box3dFrame>(); p.nframes = (int)tab.size(); p.frame_offset = frame_offset;
    p.depth = depth_code; p.NC = h->NC;
    p.part_offset = h->dc_part_offset.p; p.parent = h->dc_parent.p; p.norm = h->dc_norm.p; p.zfactor = zfactor;
    p.med = reinterpret_cast<double *>(w); w += s_med;
    p.queue = reinterpret_cast<int *>(w); w += s_queue;
    p.qn = reinterpret_cast<int *>(w); w += s_qn;
    p.flag = reinterpret_cast<int *>(w); w += s_flag;
    p.blk = reinterpret_cast<int *>(w);
    p.task_cap = tasks;
    p.out = d_out; p.out_cap = std::max(out_cap, 0);
    HIPCHK(h, hipMemsetAsync(p.qn, 0, 8 * sizeof(int), h->stream));
    static const int ids[kDcSteps] = {PBD_K_DC_CLASSIFY, PBD_K_DC_SELECT, PBD_K_DC_COMPACT};
    for (int step = 0; step < kDcSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_depth_consistency(p, h->f64, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- suppression of a caller's list (pbd_suppress*): the canvas tables of its frame sizes, kept for the next call of the
// same sizes
int get_suppress_plan(pbd_handle *h, int nframes, const int *rows, const int *cols, Plan **out)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    std::vector<int> key;
    for (int f = 0; f < nframes; ++f) {
        if (rows[f] < 1 || cols[f] < 1 || rows[f] > 65536 || cols[f] > 65536)
            return fail(h, PBD_ERR_INVALID, "frame %d: size %dx%d (1..65536)", f, rows[f], cols[f]);
        key.push_back(rows[f]); key.push_back(cols[f]);
    }
    if (h->sup_plan && h->sup_plan->key_dims == key) { *out = h->sup_plan.get(); return PBD_OK; }
    if (h->sup_plan) HIPCHK(h, hipStreamSynchronize(h->stream));   // the previous tables may still be read
    auto M = std::make_unique<Plan>();
    M->kind = 4; M->key_dims = key; M->mixed_frames = nframes;
    for (int f = 0; f < nframes; ++f) M->fdim.push_back(make_int2(rows[f], cols[f]));
    post_canvas_plan(*M);
    h->sup_plan.reset();
    HIPCHK(h, M->d_fdim.upload(M->fdim));
    HIPCHK(h, M->d_fcanvas.upload(M->fcanvas));
    HIPCHK(h, M->d_post_lds.upload(M->post_lds));
    HIPCHK(h, M->d_post_glb.upload(M->post_glb));
    h->sup_plan = std::move(M);
    *out = h->sup_plan.get();
    return PBD_OK;
}

// the host forms: records into a payload of the handle's (word 0 = ncand), then, after `run` enqueued the stage into `dout`,
// the kept count and min(kept, capacity) records back into out
template <class Run>
int host_list_call(pbd_handle *h, DevBuf &din, DevBuf &dout, const int32_t *cand, int ncand, int32_t *out, int capacity, int *nout,
                   Run run)
{
    const size_t stride = (size_t)::stride(h);
    HIPCHK(h, din.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    HIPCHK(h, dout.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    HIPCHK(h, hipMemcpyAsync(din.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (ncand) HIPCHK(h, hipMemcpyAsync(din.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                                        h->stream));
    if (int rc = run(din.as<int32_t>(), dout.as<int32_t>())) return rc;
    int kept = 0;
    HIPCHK(h, hipMemcpyAsync(&kept, dout.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    const int nret = std::min(std::max(kept, 0), capacity);
    if (nret > 0)
        HIPCHK(h, hipMemcpy(out, dout.as<int32_t>() + 1, (size_t)nret * stride * sizeof(int32_t), hipMemcpyDeviceToHost));
    *nout = kept;
    if (kept > capacity) return fail(h, PBD_ERR_CAPACITY, "%d records kept, capacity %d", kept, capacity);
    return PBD_OK;
}

// ---- camera boxes and part centres (pbd_boxes3d_camera*; pbd_kernels_cloud.hip)
int check_camera(pbd_handle *h, int nframes, int depth_code, const pbd_pinhole *cams, int parts_mode)
{
    if (depth_code != kDepth32F) return fail(h, PBD_ERR_UNSUPPORTED, "depth code %d: the part centres read 32F depth (5)", depth_code);
    if (parts_mode != PBD_PARTS_LITERAL && parts_mode != PBD_PARTS_XY)
        return fail(h, PBD_ERR_INVALID, "parts mode %d: PBD_PARTS_LITERAL (0) or PBD_PARTS_XY (1)", parts_mode);
    for (int f = 0; f < nframes; ++f)
        if (!std::isfinite(cams[f].fx) || !std::isfinite(cams[f].fy) || cams[f].fx == 0 || cams[f].fy == 0)
            return fail(h, PBD_ERR_INVALID, "frame %d: fx %g, fy %g (finite, non-zero)", f, cams[f].fx, cams[f].fy);
    return PBD_OK;
}

// k_boxes3d into the handle's cube buffer, then the camera kernel, on the handle's stream
int enqueue_camera(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, const pbd_pinhole *cams, int parts_mode,
                   const int32_t *d_payload, int capacity, int frame_offset, double *d_box, float *d_centres, int32_t *d_ncentres,
                   int32_t *d_dense)
{
    static_assert(sizeof(pbd_pinhole) == sizeof(Pinhole), "pbd_pinhole is the kernels' Pinhole");
    HIPCHK(h, h->cam_cube.ensure((size_t)capacity * 6 * sizeof(double)));
    if (int rc = enqueue_boxes3d(h, tab, depth_code, d_payload, capacity, frame_offset, h->cam_cube.as<double>())) return rc;
    if (int rc = stage_table(h, h->cam_tab_host, h->cam_tab, h->cam_tab_copied, cams, tab.size() * sizeof(Pinhole))) return rc;
    CameraParams cp{};
    cp.in = d_payload; cp.in_cap = capacity; cp.stride = stride(h); cp.max_parts = h->max_parts;
    cp.frames = h->b3_tab.as<Box3dFrame>(); cp.cams = h->cam_tab.as<Pinhole>();
    cp.nframes = (int)tab.size(); cp.frame_offset = frame_offset; cp.mode = parts_mode;
    cp.cube = h->cam_cube.as<double>();
    cp.box = d_box; cp.centres = d_centres; cp.ncentres = d_ncentres; cp.dense = d_dense;
    {
        ProfScope ps(h, PBD_K_CAMERA_BOXES, h->stream);
        launch_camera_boxes(cp, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- candidate mask (pbd_candidate_mask*; pbd_kernels_publish.hip)
// every check of a call's frames before anything is enqueued
int check_mask_frames(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, uint8_t *const *labels, const size_t *label_pitch,
                      int channels, const uint8_t *const *colour, const size_t *colour_pitch, uint8_t *const *masked,
                      const size_t *masked_pitch)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (masked && channels != 1 && channels != 3 && channels != 4)
        return fail(h, PBD_ERR_INVALID, "channels %d: 1, 3 or 4", channels);
    if ((labels && !label_pitch) || (masked && (!masked_pitch || !colour || !colour_pitch)))
        return fail(h, PBD_ERR_INVALID, "an output without its pitches or colour frames");
    for (int f = 0; f < nframes; ++f) {
        if (im_rows[f] < 1 || im_cols[f] < 1 || im_rows[f] > 65536 || im_cols[f] > 65536)
            return fail(h, PBD_ERR_INVALID, "frame %d: size %dx%d (1..65536)", f, im_rows[f], im_cols[f]);
        const size_t row = (size_t)im_cols[f];
        if (labels && (!labels[f] || label_pitch[f] < row))
            return fail(h, PBD_ERR_INVALID, "frame %d: labels %p, pitch %zu < row bytes %zu", f, (const void *)labels[f], label_pitch[f], row);
        if (masked && (!masked[f] || !colour[f] || colour_pitch[f] < row * channels || masked_pitch[f] < row * channels))
            return fail(h, PBD_ERR_INVALID, "frame %d: colour %p / masked %p, pitches %zu / %zu < row bytes %zu", f,
                        (const void *)colour[f], (const void *)masked[f], colour_pitch[f], masked_pitch[f], row * channels);
    }
    return PBD_OK;
}

// the frame table (tile numbering filled in) to the device, then the hull and the tile kernels, on the handle's stream
int enqueue_mask(pbd_handle *h, std::vector<MaskFrame> &tab, int channels, const int32_t *d_payload, int capacity, int frame_offset,
                 int32_t *d_status)
{
    long long tiles = 0;
    for (MaskFrame &fr : tab) {
        fr.tile0 = (int)tiles;
        tiles += mask_tiles(fr.rows, fr.cols);
        if (tiles > 0x7fffffffll) return fail(h, PBD_ERR_INVALID, "%zu frames: 2^31 or more pixel tiles", tab.size());
    }
    if (int rc = stage_table(h, h->mk_tab_host, h->mk_tab, h->mk_tab_copied, tab.data(), tab.size() * sizeof(MaskFrame))) return rc;
    const size_t hull_bytes = ((size_t)capacity * sizeof(int4) + 255) / 256 * 256;
    HIPCHK(h, h->mk_ws.ensure(hull_bytes + (2 * tab.size() + 1) * sizeof(int32_t)));
    MaskParams mp{};
    mp.in = d_payload; mp.in_cap = capacity; mp.stride = stride(h); mp.max_parts = h->max_parts;
    mp.frames = h->mk_tab.as<MaskFrame>(); mp.nframes = (int)tab.size(); mp.frame_offset = frame_offset;
    mp.ntiles = (int)tiles; mp.channels = channels;
    mp.hull = h->mk_ws.as<int4>();
    mp.range = reinterpret_cast<int32_t *>(h->mk_ws.as<uint8_t>() + hull_bytes);
    mp.bad = mp.range + 2 * tab.size();
    mp.status = d_status;
    {
        ProfScope ps(h, PBD_K_MK_HULL, h->stream);
        launch_mask(mp, kMkStepHull, h->stream);
    }
    {
        ProfScope ps(h, PBD_K_MK_TILE, h->stream);
        launch_mask(mp, kMkStepTile, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- part-centre poses (pbd_part_poses*; pbd_kernels_publish.hip)
int enqueue_poses(pbd_handle *h, const int32_t *d_word, int capacity, const float *d_centres, const int32_t *d_ncentres,
                  const int32_t *d_dense, int32_t *d_count, float *d_position, float *d_orientation, float *d_eigenvalues)
{
    PoseParams pp{};
    pp.count_word = d_word; pp.cap = capacity; pp.max_parts = h->max_parts;
    pp.centres = d_centres; pp.ncentres = d_ncentres; pp.dense = d_dense;
    pp.count = d_count; pp.position = d_position; pp.orientation = d_orientation; pp.eigenvalues = d_eigenvalues;
    {
        ProfScope ps(h, PBD_K_PART_POSES, h->stream);
        launch_part_poses(pp, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- object clusters (pbd_cluster_objects*; pbd_kernels_cloud.hip)
int check_clouds(pbd_handle *h, int nclouds, const pbd_cloud *c, bool host)
{
    if (nclouds < 1) return fail(h, PBD_ERR_INVALID, "nclouds %d", nclouds);
    for (int f = 0; f < nclouds; ++f) {
        if (!c[f].data || c[f].rows < 1 || c[f].cols < 1 || (long long)c[f].rows * c[f].cols >= (1LL << 31))
            return fail(h, PBD_ERR_INVALID, "cloud %d: %dx%d at %p", f, c[f].rows, c[f].cols, c[f].data);
        if (c[f].point_stride < 3 * sizeof(float))
            return fail(h, PBD_ERR_INVALID, "cloud %d: point stride %zu < 12", f, c[f].point_stride);
        const size_t row_bytes = (size_t)(c[f].cols - 1) * c[f].point_stride + 3 * sizeof(float);
        if (c[f].rows > 1 && c[f].row_stride < row_bytes)
            return fail(h, PBD_ERR_INVALID, "cloud %d: row stride %zu < row bytes %zu", f, c[f].row_stride, row_bytes);
        if (!host && (reinterpret_cast<uintptr_t>(c[f].data) % 4 || c[f].point_stride % 4 || c[f].row_stride % 4))
            return fail(h, PBD_ERR_INVALID, "cloud %d: device pointer %p / strides %zu, %zu not multiples of 4", f, c[f].data,
                        c[f].point_stride, c[f].row_stride);
    }
    return PBD_OK;
}

// the clustering workspace for `capacity` boxes, clouds of at most maxpts points and crop_cap cropped points: the bucket table
// (tcap buckets, a power of two >= 2 crop_cap), the scan partials, and one 256-byte aligned piece per array, in the order
// enqueue_cluster carves them.  crop_cap <= kClMaxCrop keeps tcap, every bucket index and every count inside an int.
constexpr long long kClMaxCrop = 1LL << 29;
constexpr int kClPieces = 14;
struct ClusterLayout {
    int nchunks;
    long long units, tcap, nparts, total;
    long long sizes[kClPieces];
};
int cluster_layout(int capacity, long long maxpts, long long crop_cap, ClusterLayout &L)
{
    if (capacity < 0 || maxpts < 1 || crop_cap < 0 || crop_cap > kClMaxCrop) return PBD_ERR_INVALID;
    L.nchunks = (int)((maxpts + kClChunk - 1) / kClChunk);
    L.units = (long long)capacity * L.nchunks;
    L.tcap = 2;
    while (L.tcap < 2 * crop_cap) L.tcap <<= 1;
    L.nparts = std::max(L.units + 1, L.tcap + 1) / (4 * 256) + 2;
    const long long c = crop_cap;
    const long long sizes[kClPieces] = {(L.units + 1) * 8, L.nparts * 8, c * 4, c * 4, c * 16, c * 4, c * 4, c * 4, c * 4, (L.tcap + 1) * 4,
                                        (L.tcap + 1) * 4, (long long)capacity * 8, (long long)capacity * 8, 4 * 8};
    L.total = 0;
    for (int i = 0; i < kClPieces; ++i) {
        L.sizes[i] = sizes[i];
        L.total += (sizes[i] + 255) / 256 * 256;
    }
    return PBD_OK;
}

// the workspace (cluster_layout), the cloud table, and the fixed sequence of launches
int enqueue_cluster(pbd_handle *h, const std::vector<CloudFrame> &tab, const int32_t *d_payload, int capacity, int rec_stride,
                    int frame_offset, const double *d_boxes, int crop_cap, int index_cap, float *d_centres, int32_t *d_counts,
                    int32_t *d_indices, long long *d_status)
{
    long long maxpts = 1;
    for (const CloudFrame &c : tab) maxpts = std::max(maxpts, (long long)c.rows * c.cols);
    ClusterLayout L;
    if (cluster_layout(capacity, maxpts, crop_cap, L))
        return fail(h, PBD_ERR_INVALID, "crop capacity %d (at most 2^29), capacity %d", crop_cap, capacity);
    const int nchunks = L.nchunks;
    const long long tcap = L.tcap, total = L.total;
    const long long *sizes = L.sizes;
    HIPCHK(h, h->cl_ws.ensure((size_t)total));
    if (int rc = stage_table(h, h->cl_tab_host, h->cl_tab, h->cl_tab_copied, tab.data(), tab.size() * sizeof(CloudFrame))) return rc;
    uint8_t *w = h->cl_ws.as<uint8_t>();
    int piece = 0;
    auto carve = [&]() { uint8_t *p = w; w += (sizes[piece++] + 255) / 256 * 256; return (void *)p; };
    ClusterParams p{};
    p.in = d_payload; p.in_cap = capacity; p.rec_stride = rec_stride; p.frame_offset = frame_offset;
    p.clouds = h->cl_tab.as<CloudFrame>(); p.nclouds = (int)tab.size(); p.nchunks = nchunks;
    p.boxes = d_boxes; p.crop_cap = crop_cap; p.index_cap = index_cap;
    p.chunk_off = (long long *)carve(); p.part = (long long *)carve();
    p.crop_idx = (int32_t *)carve(); p.crop_box = (int32_t *)carve(); p.crop_xyz = (float4 *)carve();
    p.bucket = (int32_t *)carve(); p.parent = (int32_t *)carve(); p.csize = (int32_t *)carve(); p.sorted = (int32_t *)carve();
    p.bstart = (int32_t *)carve(); p.bcur = (int32_t *)carve(); p.tcap = (int)tcap;      // <= 2^30 (cluster_layout)
    p.best = (unsigned long long *)carve(); p.obase = (long long *)carve(); p.ntab = (long long *)carve();
    p.centres = d_centres; p.counts = d_counts; p.indices = d_indices; p.status = d_status;
    static const int ids[kClSteps] = {PBD_K_CL_CROP_COUNT, PBD_K_CL_CROP_SCAN, PBD_K_CL_CROP_SCATTER, PBD_K_CL_CLEAR, PBD_K_CL_GRID_COUNT,
                                      PBD_K_CL_GRID_SCAN, PBD_K_CL_GRID_SCATTER, PBD_K_CL_HOOK, PBD_K_CL_LABEL, PBD_K_CL_BEST,
                                      PBD_K_CL_SELECT, PBD_K_CL_OUT};
    for (int step = 0; step < kClSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_cluster_step(p, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- plane removal (pbd_remove_planes*; pbd_kernels_planes.hip)
// the reference's call (include/PointCloudClusterer.hpp:294-336 with PCL's defaults): see include/pbd.h
pbd_plane_params plane_defaults()
{
    pbd_plane_params q;
    q.smoothing_size = 10;
    q.depth_change_factor = 0.02f;
    q.distance_threshold = 0.02f;
    q.angular_threshold = 3.0 * M_PI / 180.0;
    q.max_curvature = 0.001;
    q.min_inliers = 1000;
    q.refine = 1;
    return q;
}

int check_plane_params(pbd_handle *h, const pbd_plane_params &q)
{
    if (q.smoothing_size < 2 || q.smoothing_size > 128 || q.min_inliers < 0 || !std::isfinite(q.depth_change_factor) ||
        !std::isfinite(q.distance_threshold) || !std::isfinite(q.angular_threshold) || !std::isfinite(q.max_curvature) ||
        (q.refine != 0 && q.refine != 1))
        return fail(h, PBD_ERR_INVALID, "plane parameters: smoothing size %d (2..128), min inliers %d (>= 0), refine %d (0 or 1), "
                    "every threshold finite", q.smoothing_size, q.min_inliers, q.refine);
    return PBD_OK;
}

// organized clouds: the pbd_cloud rules, rows >= 2 and cols >= 2, and fewer than 2^31 points in the whole call
int check_organized(pbd_handle *h, int nclouds, const pbd_cloud *c, bool host)
{
    if (int rc = check_clouds(h, nclouds, c, host)) return rc;
    long long total = 0;
    for (int f = 0; f < nclouds; ++f) {
        if (c[f].rows < 2 || c[f].cols < 2)
            return fail(h, PBD_ERR_INVALID, "cloud %d: %dx%d is not organized (rows and cols >= 2)", f, c[f].rows, c[f].cols);
        total += (long long)c[f].rows * c[f].cols;
    }
    if (total >= (1LL << 31)) return fail(h, PBD_ERR_INVALID, "the clouds of one call hold %lld points (below 2^31)", total);
    return PBD_OK;
}

// the plane-removal workspace: one 256-byte aligned piece per array, in the order enqueue_planes carves them.  cand_cap bounds the
// segments above min_inliers: at most points / (min_inliers + 1) per cloud
constexpr int kPlPieces = 17;
struct PlaneLayout {
    long long cand_cap, total;
    long long sizes[kPlPieces];
};
void plane_layout(int nclouds, long long npts, long long nrows, long long cand_cap, PlaneLayout &L)
{
    const long long n = npts, c = cand_cap + 1, tiles = (n + 1023) / 1024 + 2;
    const long long sizes[kPlPieces] = {n * 16, n * 16, n * 16, n * 16, n * 4, n * 4, (n + 1) * 4, n * 4, tiles * 8, c * 4, c * 4,
                                        c * 4, c * 16, c * 16, ((long long)nclouds + 1) * 4, (long long)nclouds * 4, 2 * nrows * 8};
    L.cand_cap = cand_cap;
    L.total = 0;
    for (int i = 0; i < kPlPieces; ++i) {
        L.sizes[i] = sizes[i];
        L.total += (sizes[i] + 255) / 256 * 256;
    }
}

// the workspace, the cloud table and the fixed sequence of launches; outputs as pbd_remove_planes_device
int enqueue_planes(pbd_handle *h, const std::vector<PlaneCloud> &tab, const pbd_plane_params &q, float *d_points, int32_t *d_kept,
                   int32_t *d_nkept, int32_t *d_labels, float *d_planes, int32_t *d_inliers, int32_t *d_nplanes, int plane_cap,
                   long long *d_status)
{
    const int nclouds = (int)tab.size() - 1;
    long long cand_cap = 0, nrows = 0;
    for (int i = 0; i < nclouds; ++i) {
        cand_cap += (long long)tab[i].rows * tab[i].cols / ((long long)q.min_inliers + 1);
        nrows += tab[i].rows;
    }
    const long long npts = tab[nclouds].base;
    PlaneLayout L;
    plane_layout(nclouds, npts, nrows, cand_cap, L);
    HIPCHK(h, h->pl_ws.ensure((size_t)L.total));
    if (int rc = stage_table(h, h->pl_tab_host, h->pl_tab, h->pl_tab_copied, tab.data(), tab.size() * sizeof(PlaneCloud))) return rc;
    uint8_t *w = h->pl_ws.as<uint8_t>();
    int piece = 0;
    auto carve = [&]() { uint8_t *ptr = w; w += (L.sizes[piece++] + 255) / 256 * 256; return (void *)ptr; };
    PlaneParams p{};
    p.clouds = h->pl_tab.as<PlaneCloud>(); p.nclouds = nclouds; p.npts = npts;
    p.half = q.smoothing_size / 2;
    p.depth_change = q.depth_change_factor; p.dist_thr = q.distance_threshold;
    p.cos_thr = (float)cos(q.angular_threshold);
    p.max_curv = q.max_curvature; p.min_inliers = q.min_inliers;
    p.plane_cap = plane_cap; p.cand_cap = (int)std::min<long long>(cand_cap, INT32_MAX);
    p.xyz = (float4 *)carve(); p.rsx = (float4 *)carve(); p.rsy = (float4 *)carve(); p.nrm = (float4 *)carve();
    p.parent = (int32_t *)carve(); p.csize = (int32_t *)carve(); p.flag = (int32_t *)carve(); p.lab = (int32_t *)carve();
    p.part = (long long *)carve();
    p.cand_root = (int32_t *)carve(); p.cand_plane = (int32_t *)carve(); p.plane_cnt = (int32_t *)carve();
    p.cand_coef = (float4 *)carve(); p.plane_coef = (float4 *)carve();
    p.cbase = (int32_t *)carve(); p.np = (int32_t *)carve(); p.xch = (int2 *)carve();
    p.points = d_points; p.kept = d_kept; p.nkept = d_nkept; p.labels = d_labels; p.planes = d_planes; p.inliers = d_inliers;
    p.nplanes = d_nplanes; p.status = d_status;
    for (int step = 0; step < kPlSteps; ++step)
        if (step != kPlStepRefine || q.refine) launch_planes_step(p, step, h->stream);
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the cloud table of a call: every cloud's place in the concatenation, one closing entry holding the point total
std::vector<PlaneCloud> plane_table(int nclouds, const pbd_cloud *c)
{
    std::vector<PlaneCloud> tab(nclouds + 1);
    long long base = 0, rbase = 0;
    for (int f = 0; f < nclouds; ++f) {
        tab[f] = PlaneCloud{static_cast<const uint8_t *>(c[f].data), c[f].rows, c[f].cols, (long long)c[f].point_stride,
                            (long long)c[f].row_stride, base, rbase};
        base += (long long)c[f].rows * c[f].cols;
        rbase += c[f].rows;
    }
    tab[nclouds] = PlaneCloud{nullptr, 0, 0, 0, 0, base, rbase};
    return tab;
}

// a (frame, level) of the resident result -> (frame index into the buffers, level of the plan); mixed plans: frame 0, the
// frame's level in the virtual table
bool resident_level(const Resident &r, int frame, int level, int *bf, int *bl)
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

// pbd_examples*: the resident result a record can be walked in (PBD_OK or the failure's status code)
// the handle whose buffers hold the resident result: the latent twin after pbd_detect_latent
pbd_handle *resident_owner(pbd_handle *h) { return h->res.latent && h->lat ? h->lat.get() : h; }

int check_examples_state(pbd_handle *h)
{
    const Resident &r = resident_owner(h)->res;
    if (!r.plan || (r.plan->kind != 0 && r.plan->kind != 2) || !r.features || !r.dp)
        return fail(h, PBD_ERR_STATE, "no resident detect result (pbd_detect* computes one; pbd_dp_min and pbd_conv_set_filters leave none)");
    if (!h->bank_matches_model || h->filter_ksize != h->model_ksize)
        return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's: the model vector no longer describes it");
    return PBD_OK;
}

// the walk and the gather of min(max(word 0, 0), capacity) records of d_in into d_hdr / d_values, on the handle's stream
int enqueue_examples(pbd_handle *h, const int32_t *d_in, int capacity, int frame_offset, int32_t *d_hdr, void *d_values)
{
    pbd_handle *o = resident_owner(h);   // its maps and features; the model tables (filter ids, offsets) stay this handle's
    Plan &P = *o->res.plan;
    if (!h->ex_gm.p) {
        std::vector<ExGm> gm(h->totmix);
        for (int i = 0; i < h->totmix; ++i) gm[i] = ExGm{h->filterid[i], h->biasid[i], h->defid[i], 0};
        HIPCHK(h, h->ex_gm.upload(gm));
        std::vector<int> anc(h->anchors);
        anc.push_back(0);
        HIPCHK(h, h->ex_anchors.upload(anc));
        HIPCHK(h, h->ex_foff.upload(h->model_foff));
    }
    if (P.kind == 2 && !P.d_frame_lv0.p) HIPCHK(h, P.d_frame_lv0.upload(P.frame_lv0));
    HIPCHK(h, h->ex_ws.ensure(std::max<size_t>((size_t)capacity * h->max_parts * sizeof(ExPart), 16)));
    ExampleParams ep{};
    ep.in = d_in; ep.in_cap = capacity; ep.stride = stride(h); ep.frame_offset = frame_offset;
    ep.lv = P.d_lv.p; ep.nlevels = P.nlevels;
    ep.nframes = P.kind == 2 ? P.mixed_frames : o->res.frames;
    ep.frame_lv0 = P.kind == 2 ? P.d_frame_lv0.p : nullptr;
    ep.cell_per_frame = P.cell_per_frame;
    ep.NC = h->NC; ep.NS = h->NS; ep.NJ = h->totmix; ep.ptr8 = P.ptr8 ? 1 : 0; ep.flen = 32; ep.max_parts = h->max_parts;
    ep.rooti = o->rooti.as<int>(); ep.IxRaw = o->IxRaw.p; ep.IyRaw = o->IyRaw.p; ep.Ik = o->Ik.as<uint8_t>();
    ep.walk = h->d_walk.p; ep.walk_off = h->d_walk_off.p;
    ep.gm = h->ex_gm.p; ep.anchors = h->ex_anchors.p; ep.foff = h->ex_foff.p; ep.nbias = h->nbias; ep.ndefs = h->ndefs;
    ep.feat = o->feat.p;
    ep.parts = h->ex_ws.as<ExPart>();
    ep.hdr = d_hdr; ep.hdr_words = h->ex_hdr_words;
    ep.values = d_values; ep.vstride = h->ex_values;
    { ProfScope ps(h, PBD_K_EX_WALK, h->stream); launch_examples(ep, h->f64, 0, h->stream); }
    { ProfScope ps(h, PBD_K_EX_GATHER, h->stream); launch_examples(ep, h->f64, 1, h->stream); }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

const char *pbd_version(void) { return "pbd-hip 0.1 (gfx950)"; }

// diagnostics, not part of include/pbd.h
int pbd_debug_conv_occupancy(int nw) { return nw == 5 ? conv_mfma_occupancy(false) : nw == 6 ? conv_mfma_occupancy(true) : conv_occupancy(nw); }
// the clustering workspace of pbd_cluster_objects* (host-only, no GPU needed): out = {nchunks, units, tcap, nparts, total, the
// 14 piece sizes}; PBD_ERR_INVALID for a crop capacity the calls refuse
int pbd_debug_cluster_layout(int capacity, long long maxpts, long long crop_cap, long long *out)
{
    ClusterLayout L;
    if (int rc = cluster_layout(capacity, maxpts, crop_cap, L)) return rc;
    out[0] = L.nchunks; out[1] = L.units; out[2] = L.tcap; out[3] = L.nparts; out[4] = L.total;
    for (int i = 0; i < kClPieces; ++i) out[5 + i] = L.sizes[i];
    return PBD_OK;
}
// the convolution's tile cover of one rows x cols level (host-only, no GPU needed): out[i] = {shape, y0, x0}
int pbd_debug_cover_level(int rows, int cols, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        std::vector<ConvTile> shaped[3];
        cover_level(0, rows, cols, shaped);
        int n = 0;
        for (int k = 0; k < 3; ++k)
            for (const ConvTile &t : shaped[k]) {
                if (n < capacity) { out[3 * n] = k; out[3 * n + 1] = t.y0; out[3 * n + 2] = t.x0; }
                ++n;
            }
        return n;
    });
}

// the exact convolution's strip-sequence tiles for `nb` frames of the given feature-map sizes (host-only, no GPU needed):
// out[i] = {nseg, len0, len1, len2, then per segment frame, level, strip, x0} = 16 ints per tile; returns the tile count
int pbd_debug_seg_tiles(int nlevels, const int *rows, const int *cols, int nb, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        std::vector<LevelDesc> lv(nlevels);
        for (int l = 0; l < nlevels; ++l) { memset(&lv[l], 0, sizeof lv[l]); lv[l].rows = rows[l]; lv[l].cols = cols[l]; }
        std::vector<ConvSegTile> tiles;
        build_seg_tiles(lv, nb, tiles);
        static_assert(sizeof(ConvSegTile) == 16 * sizeof(int), "a tile record is 16 ints");
        for (size_t i = 0; i < tiles.size() && (int)i < capacity; ++i) memcpy(out + 16 * i, &tiles[i], sizeof(ConvSegTile));
        return (int)tiles.size();
    });
}

// the virtual level table of a mixed-size call (host-only, no GPU needed): frames of rows[f] x cols[f] in call order, for a
// model of `sbin` / `interval`; out[i] = {frame, local level, img_rows, img_cols, rows, cols, cell_off} = 7 ints per level
// (cell_off fits an int for every frame size accepted); returns the level count, or PBD_ERR_INVALID (a frame too small)
int pbd_debug_mixed_plan(int sbin, int interval, int nframes, const int *rows, const int *cols, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        if (nframes < 1 || sbin < 2 || interval < 1 || !rows || !cols) return PBD_ERR_INVALID;
        Plan M;
        for (int f = 0; f < nframes; ++f) {
            Plan Q;
            std::string err;
            if (rows[f] < 1 || cols[f] < 1 || image_plan_host(rows[f], cols[f], sbin, interval, Q, err)) return PBD_ERR_INVALID;
            mixed_append(M, Q);
        }
        mixed_finish(M, interval);
        for (int l = 0; l < M.nlevels && l < capacity; ++l) {
            const LevelDesc &d = M.lv[l];
            int *o = out + 7 * (size_t)l;
            o[0] = M.lv_frame[l]; o[1] = M.lv_local[l]; o[2] = d.img_rows; o[3] = d.img_cols; o[4] = d.rows; o[5] = d.cols;
            o[6] = (int)d.cell_off;
        }
        return M.nlevels;
    });
}

// runs a body that throws inside the ABI guard (host-only): 0 = std::bad_alloc, 1 = std::length_error from an absurd
// std::vector size, 2 = another std::exception; returns the status code the guard produced
int pbd_debug_guard_selftest(int kind)
{
    return guarded(nullptr, [&]() -> int {
        if (kind == 0) throw std::bad_alloc();
        if (kind == 1) { std::vector<int32_t> v; v.resize(v.max_size() + (size_t)1); return (int)v.size(); }
        if (kind == 2) throw std::runtime_error("selftest");
        return PBD_OK;
    });
}

// the post-processing stage of pbd_set_nms on a caller-built record list (tests: exact ties, boxes outside the frame, very
// long lists): records[n] grouped by ascending frame (frames 0..), each with 1..max_parts parts; out receives min(kept,
// capacity) records, *nout = that count; PBD_ERR_CAPACITY when more were kept
int pbd_debug_postprocess(pbd_handle *h, int rows, int cols, const int32_t *records, int n, float overlap, int32_t *out, int capacity,
                          int *nout)
{
    return entry(h, nout && (n <= 0 || records) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (rows < 1 || cols < 1 || rows > 65536 || cols > 65536 || n < 0 || capacity < 0 || std::isnan(overlap))
            return fail(h, PBD_ERR_INVALID, "rows %d, cols %d, n %d, capacity %d", rows, cols, n, capacity);
        const int stride = ::stride(h);
        int nframes = 1;
        for (int i = 0; i < n; ++i) {
            const int32_t *r = records + (size_t)i * stride;
            if (r[0] < 0 || (i > 0 && r[0] < records[(size_t)(i - 1) * stride]) || r[6] < 1 || r[6] > h->max_parts)
                return fail(h, PBD_ERR_INVALID, "record %d: frame %d, nparts %d (frames ascending from 0, 1..%d parts)", i, r[0], r[6],
                            h->max_parts);
            nframes = r[0] + 1;
        }
        if (nframes > 65536) return fail(h, PBD_ERR_INVALID, "%d frames", nframes);
        const int in_cap = std::max(n, 1);
        HIPCHK(h, h->dbg_in.ensure(((size_t)in_cap * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, h->dbg_out.ensure(((size_t)capacity * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(h->dbg_in.p, &n, sizeof(int32_t), hipMemcpyHostToDevice));
        if (n) HIPCHK(h, hipMemcpy(h->dbg_in.as<int32_t>() + 1, records, (size_t)n * stride * sizeof(int32_t), hipMemcpyHostToDevice));
        if (int rc = enqueue_post(h, nframes, rows, cols, overlap, h->dbg_in.as<int32_t>(), in_cap, 0, h->dbg_out.as<int32_t>(), capacity,
                              h->stream)) return rc;
        HIPCHK(h, hipGetLastError());
        int kept = 0;
        HIPCHK(h, hipMemcpyAsync(&kept, h->dbg_out.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int nret = std::min(kept, capacity);
        if (nret > 0) HIPCHK(h, hipMemcpy(out, h->dbg_out.as<int32_t>() + 1, (size_t)nret * stride * sizeof(int32_t), hipMemcpyDeviceToHost));
        *nout = nret;
        if (kept > capacity) return fail(h, PBD_ERR_CAPACITY, "%d records kept, capacity %d", kept, capacity);
        return PBD_OK;
    });
}

// forces one of the handle's launch choices (tests: every distance-transform variant, DP chunking on small batches);
// each option's default value restores the automatic choice
enum { PBD_DEBUG_DT_LANE_SHIFT = 0, PBD_DEBUG_DT_COOP = 1, PBD_DEBUG_DT_COOP_G = 2, PBD_DEBUG_DP_BUDGET_MB = 3 };
int pbd_debug_set_option(pbd_handle *h, int option, int value)
{
    return entry(h, true, kIdle, [&]() -> int {
        switch (option) {
        case PBD_DEBUG_DT_LANE_SHIFT:   // 0..6: 64 >> value rows per wave; -1: automatic
            if (value < -1 || value > 6) break;
            h->dt_opt.lane_shift = value;
            return PBD_OK;
        case PBD_DEBUG_DT_COOP:         // 0: never the cooperative kernel; 1: when it fits
            if (value != 0 && value != 1) break;
            h->dt_opt.coop = value != 0;
            return PBD_OK;
        case PBD_DEBUG_DT_COOP_G:       // 4 or 8 rows per wave of the cooperative kernel; 0: automatic
            if (value != 0 && value != 4 && value != 8) break;
            h->dt_opt.coop_g = value;
            return PBD_OK;
        case PBD_DEBUG_DP_BUDGET_MB:    // DP scratch per chunk of frames in MB; 0: 8 GB
            if (value < 0) break;
            h->dp_budget_mb = value;
            return PBD_OK;
        default:
            return fail(h, PBD_ERR_INVALID, "debug option %d unknown", option);
        }
        return fail(h, PBD_ERR_INVALID, "debug option %d: value %d out of range", option, value);
    });
}

const char *pbd_last_error(const pbd_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pbd_create(const pbd_model *model, const pbd_config *config, pbd_handle **out)
{
    return guarded(nullptr, [&]() -> int {
        if (!model || !config || !out) return fail(nullptr, PBD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (config->real_type != PBD_REAL_F32 && config->real_type != PBD_REAL_F64)
            return fail(nullptr, PBD_ERR_UNSUPPORTED, "real_type %d: PBD_REAL_F32 or PBD_REAL_F64", config->real_type);
        if (config->conv_mode == PBD_CONV_MFMA_F64 && config->real_type != PBD_REAL_F64)
            return fail(nullptr, PBD_ERR_UNSUPPORTED, "PBD_CONV_MFMA_F64 needs PBD_REAL_F64 (fp64 operands and accumulation)");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev < 1)
            return fail(nullptr, PBD_ERR_HIP, "no HIP device available (%s); this library has no CPU path",
                        e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        if (config->device < 0 || config->device >= ndev) return fail(nullptr, PBD_ERR_INVALID, "device %d of %d", config->device, ndev);
        e = hipSetDevice(config->device);
        if (e != hipSuccess) return fail(nullptr, PBD_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
        std::unique_ptr<pbd_handle, void (*)(pbd_handle *)> h(new pbd_handle, pbd_destroy);   // releases device memory on every exit
        h->cfg = *config;
        h->f64 = config->real_type == PBD_REAL_F64;
        h->rs = h->f64 ? sizeof(double) : sizeof(float);
        h->resp_half = config->conv_mode == PBD_CONV_MFMA_F16 && !h->f64;
        h->resp_es = h->resp_half ? 2 : h->rs;
        if (h->cfg.max_batch < 1) h->cfg.max_batch = 1;
        if (h->cfg.max_candidates < 1) h->cfg.max_candidates = 65536;
        if (config->stream) {
            h->stream.borrow(reinterpret_cast<hipStream_t>(config->stream));
        } else {
            e = h->stream.create();
            if (e != hipSuccess) return fail(nullptr, PBD_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        int rc = build_model(h.get(), model);
        if (rc != PBD_OK) {
            g_create_error = h->err;
            return rc;
        }
        *out = h.release();
        return PBD_OK;
    });
}

void pbd_destroy(pbd_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    for (hipStream_t s : {h->stream.s, h->stream_copy.s, h->stream_d2h.s})   // work in flight ends before its memory is freed
        if (s) (void)hipStreamSynchronize(s);
    try {
        h->prof.flush();
    } catch (...) {
    }
    delete h;   // the members' owners free every device, pinned, event and stream resource
}

int pbd_candidate_stride(const pbd_handle *h) { return h ? stride(h) : 0; }
int pbd_binsize(const pbd_handle *h) { return h ? h->sbin : 0; }
int pbd_num_ptr_slots(const pbd_handle *h) { return h ? h->NS : 0; }
int pbd_ptr_slot(const pbd_handle *h, int component, int part)
{
    if (!h || component < 0 || component >= h->NC) return -1;
    const int p0 = h->part_offset[component];
    if (part < 0 || p0 + part >= h->part_offset[component + 1]) return -1;
    return h->ptr_slot[p0 + part];
}

int pbd_set_level_shard(pbd_handle *h, int rank, int world)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (world < 1 || rank < 0 || rank >= world) return fail(h, PBD_ERR_INVALID, "level shard %d of %d", rank, world);
        if (world > 1 && h->nms)
            return fail(h, PBD_ERR_UNSUPPORTED, "level sharding with non-maxima suppression on: suppression of one rank's levels "
                        "is not suppression of the union (pbd_set_nms(h, 0, ...) first)");
        if (rank == h->shard_rank && world == h->shard_world) return PBD_OK;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->shard_rank = rank; h->shard_world = world;
        // image plans depend on the shard
        h->res.clear();
        for (size_t i = 0; i < h->plans.size();)
            if (h->plans[i]->kind == 0) h->plans.erase(h->plans.begin() + i); else ++i;
        return PBD_OK;
    });
}

int pbd_set_nms(pbd_handle *h, int enable, float overlap)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        if (enable && h->shard_world > 1)
            return fail(h, PBD_ERR_UNSUPPORTED, "non-maxima suppression with level sharding (world %d): suppression of one rank's "
                        "levels is not suppression of the union", h->shard_world);
        h->nms = enable != 0;
        h->nms_overlap = overlap;
        return PBD_OK;
    });
}

int pbd_pyramid_plan(pbd_handle *h, int rows, int cols, int *nlevels, int *img_rows, int *img_cols, int *feat_rows,
                     int *feat_cols, float *scales)
{
    return entry(h, nlevels, kBusyOk, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = get_image_plan(h, rows, cols, &P)) return rc;
        *nlevels = P->nlevels;
        for (int l = 0; l < P->nlevels; ++l) {
            if (img_rows) img_rows[l] = P->lv[l].img_rows;
            if (img_cols) img_cols[l] = P->lv[l].img_cols;
            if (feat_rows) feat_rows[l] = P->lv[l].rows;
            if (feat_cols) feat_cols[l] = P->lv[l].cols;
            if (scales) scales[l] = P->scales[l];
        }
        return PBD_OK;
    });
}

int pbd_features_pyramid(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes,
                         int depth_code, void *const *feat)
{
    return entry(h, img && feat, kIdle, [&]() -> int {
        const FrameSrc src{&img, stride_bytes, nullptr};
        Plan *P = nullptr;
        if (int rc = check_frames(h, 1, src, rows, cols, channels, depth_code)) return rc;
        if (int rc = get_image_plan(h, rows, cols, &P)) return rc;
        if (int rc = enqueue_features(h, *P, 1, src, channels, depth_code)) return rc;
        for (int l = 0; l < P->nlevels; ++l) {
            const LevelDesc &d = P->lv[l];
            const size_t n = (size_t)d.rows * d.cols * 32;
            if (n && feat[l])
                HIPCHK(h, hipMemcpyAsync(feat[l], h->feat.as<char>() + (size_t)d.cell_off * 32 * h->rs, n * h->rs,
                                         hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_get_pyramid_image(pbd_handle *h, int frame, int level, uint8_t *dst)
{
    return entry(h, dst, kIdle, [&]() -> int {
        const Resident &r = h->res;
        if (!r.plan || (r.plan->kind != 0 && r.plan->kind != 2) || !r.features) return fail(h, PBD_ERR_STATE, "no pyramid has been computed");
        const Plan &P = *r.plan;
        if (!resident_level(r, frame, level, &frame, &level)) return fail(h, PBD_ERR_INVALID, "frame/level out of range");
        const LevelDesc &d = P.lv[level];
        const size_t es = depth_size(r.depth);
        HIPCHK(h, hipMemcpyAsync(dst, h->pyr.as<uint8_t>() + ((size_t)frame * P.pix_per_frame + d.img_off) * r.cn * es,
                                 (size_t)d.img_rows * d.img_cols * r.cn * es, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_conv_set_filters(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    return entry(h, filters && ksize, kIdle, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (int rc = upload_filters(h, nfilters, filters, ksize)) return rc;
        h->res.drop_conv();   // the resident responses were those of the old bank
        return revalidate_bank(h);
    });
}

int pbd_conv_pdf(pbd_handle *h, int nlevels, const void *const *feat, const int *rows, const int *cols, void *const *resp)
{
    return entry(h, feat && rows && cols && resp, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = get_dims_plan(h, nlevels, rows, cols, &P)) return rc;
        h->res = Resident{P, 1};
        HIPCHK(h, h->feat.ensure(std::max<size_t>((size_t)P->cell_per_frame * 32 * h->rs, 16)));
        for (int l = 0; l < nlevels; ++l) {
            const size_t n = (size_t)rows[l] * cols[l] * 32;
            if (n) HIPCHK(h, hipMemcpyAsync(h->feat.as<char>() + (size_t)P->lv[l].cell_off * 32 * h->rs, feat[l], n * h->rs,
                                            hipMemcpyHostToDevice, h->stream));
        }
        h->res.features = true;
        if (int rc = run_conv(h, *P, 1)) return rc;
        for (int l = 0; l < nlevels; ++l) {
            const char *src = h->resp.as<char>() + (size_t)P->lv[l].cell_off * h->F * h->resp_es;
            if (int rc = read_responses(h, resp[l], src, (size_t)rows[l] * cols[l] * h->F)) return rc;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_dp_min(pbd_handle *h, int nlevels, const int *rows, const int *cols, const void *const *resp, int32_t *const *Ix,
               int32_t *const *Iy, int32_t *const *Ik, void *const *rootv, int32_t *const *rooti)
{
    return entry(h, rows && cols && resp, kIdle, [&]() -> int {
        if (int rc = check_bank(h)) return rc;
        Plan *P = nullptr;
        if (int rc = get_dims_plan(h, nlevels, rows, cols, &P)) return rc;
        h->res = Resident{P, 1};
        HIPCHK(h, h->resp.ensure(std::max<size_t>((size_t)P->cell_per_frame * h->F * h->resp_es, 16) + 32));
        std::vector<uint16_t> halfbuf;
        for (int l = 0; l < nlevels; ++l) {
            const size_t n = (size_t)rows[l] * cols[l] * h->F;
            if (!n) continue;
            char *dst = h->resp.as<char>() + (size_t)P->lv[l].cell_off * h->F * h->resp_es;
            if (h->resp_half) {      // the device side of this mode reads fp16 responses (exact for what pbd_conv_pdf returned)
                halfbuf.resize(n);
                const float *src = static_cast<const float *>(resp[l]);
                for (size_t i = 0; i < n; ++i) halfbuf[i] = host_f2h(src[i]);
                HIPCHK(h, hipMemcpy(dst, halfbuf.data(), n * 2, hipMemcpyHostToDevice));
            } else {
                HIPCHK(h, hipMemcpyAsync(dst, resp[l], n * h->rs, hipMemcpyHostToDevice, h->stream));
            }
        }
        h->res.resp = true;
        if (int rc = run_dp(h, *P, 1)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<uint8_t> t8;
        for (int l = 0; l < nlevels; ++l) {
            const size_t hw = (size_t)rows[l] * cols[l];
            if (!hw) continue;
            const size_t n = hw * h->NS, off = (size_t)P->lv[l].cell_off * h->NS;
            if (n) {
                t8.resize(n);
                // the device keeps the winning mixture per slot (Ik) and the transform's own pointer planes per (part, mixture);
                // the reference's Ix / Iy of a slot are composed here: Ix = IxRaw[k][y][x], Iy = IyRaw[k][y][Ix], k = Ik
                HIPCHK(h, hipMemcpy(t8.data(), h->Ik.as<uint8_t>() + off, n, hipMemcpyDeviceToHost));
                std::vector<uint8_t> ik(t8.begin(), t8.begin() + n);
                if (Ik && Ik[l]) for (size_t i = 0; i < n; ++i) Ik[l][i] = ik[i];
                if ((Ix && Ix[l]) || (Iy && Iy[l])) {
                    const size_t nj = hw * h->totmix, joff = (size_t)P->lv[l].cell_off * h->totmix;
                    std::vector<int> px(nj), py(nj);
                    auto fetch_planes = [&](const DevBuf &src, std::vector<int> &dst) -> hipError_t {
                        if (P->ptr8) {
                            std::vector<uint8_t> b(nj);
                            hipError_t e = hipMemcpy(b.data(), src.as<uint8_t>() + joff, nj, hipMemcpyDeviceToHost);
                            if (e != hipSuccess) return e;
                            for (size_t i = 0; i < nj; ++i) dst[i] = b[i];
                            return hipSuccess;
                        }
                        std::vector<int16_t> b(nj);
                        hipError_t e = hipMemcpy(b.data(), src.as<int16_t>() + joff, nj * 2, hipMemcpyDeviceToHost);
                        if (e != hipSuccess) return e;
                        for (size_t i = 0; i < nj; ++i) dst[i] = b[i];
                        return hipSuccess;
                    };
                    HIPCHK(h, fetch_planes(h->IxRaw, px));
                    HIPCHK(h, fetch_planes(h->IyRaw, py));
                    const int Wl = cols[l];
                    const int totparts = (int)h->parentid.size();
                    for (int gp = 0; gp < totparts; ++gp) {
                        bool root = false;
                        for (int c = 0; c < h->NC; ++c) root = root || gp == h->part_offset[c];
                        if (root) continue;
                        int c = 0;
                        while (c + 1 < h->NC && h->part_offset[c + 1] <= gp) ++c;
                        const int gpar = h->part_offset[c] + h->parentid[gp];
                        const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                        for (int pm = 0; pm < L; ++pm) {
                            const size_t so = (size_t)(h->ptr_slot[gp] + pm) * hw;
                            for (size_t cell = 0; cell < hw; ++cell) {
                                const size_t plane = (size_t)(h->mix_offset[gp] + ik[so + cell]) * hw;
                                const int x = px[plane + (cell % Wl) * (size_t)rows[l] + cell / Wl];      // IxRaw is kept transposed
                                if (Ix && Ix[l]) Ix[l][so + cell] = x;
                                if (Iy && Iy[l]) Iy[l][so + cell] = py[plane + (cell / Wl) * Wl + x];
                            }
                        }
                    }
                }
            }
            const size_t roff = (size_t)P->lv[l].cell_off * h->NC;
            if (rootv && rootv[l]) HIPCHK(h, hipMemcpy(rootv[l], h->rootv.as<char>() + roff * h->rs, hw * h->NC * h->rs, hipMemcpyDeviceToHost));
            if (rooti && rooti[l]) HIPCHK(h, hipMemcpy(rooti[l], h->rooti.as<int>() + roff, hw * h->NC * sizeof(int), hipMemcpyDeviceToHost));
        }
        return PBD_OK;
    });
}

int pbd_dp_argmin(pbd_handle *h, const float *scales, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, scales && cand && ncand, kIdle, [&]() -> int {
        if (!h->res.plan || !h->res.dp) return fail(h, PBD_ERR_STATE, "argmin() before min()");
        if (h->res.plan->kind == 2)
            return fail(h, PBD_ERR_STATE, "argmin() after a mixed-size call: DynamicProgram::argmin takes the scales of one image");
        Plan &P = *h->res.plan;
        HIPCHK(h, h->scales_tmp.ensure(sizeof(float) * PBD_MAX_LEVELS));
        HIPCHK(h, hipMemcpyAsync(h->scales_tmp.p, scales, sizeof(float) * P.nlevels, hipMemcpyHostToDevice, h->stream));
        return run_argmin(h, P, h->res.frames, h->scales_tmp.as<float>(), false, cand, capacity, ncand);   // no suppression (DynamicProgram::argmin)
    });
}

int pbd_detect(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes, int32_t *cand,
               int capacity, int *ncand)
{
    return pbd_detect_batch(h, 1, &img, rows, cols, channels, stride_bytes, cand, capacity, ncand);
}

int pbd_detect_batch(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                     size_t stride_bytes, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, imgs && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, nframes, FrameSrc{imgs, stride_bytes, nullptr}, rows, cols, channels, kDepth8U, cand, capacity, ncand);
    });
}

int pbd_detect_batch_device(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                            int32_t *cand, int capacity, int *ncand)
{
    return entry(h, d_frames && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, nframes, FrameSrc{nullptr, 0, d_frames}, rows, cols, channels, kDepth8U, cand, capacity, ncand);
    });
}

int pbd_detect_typed(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes, int depth_code,
                     int32_t *cand, int capacity, int *ncand)
{
    return entry(h, img && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, 1, FrameSrc{&img, stride_bytes, nullptr}, rows, cols, channels, depth_code, cand, capacity, ncand);
    });
}

// what submit() does once the batch has passed check_detect and its frames are (being) made resident at d_frames: the
// whole path, the candidates' read-back and the slot's completion event, all enqueued on the handle's stream without waiting
static int submit_enqueue(pbd_handle *h, pbd_handle::Slot &S, Plan &P, int nframes, const void *d_frames, int channels)
{
    if (!S.done.p) HIPCHK(h, hipEventCreateWithFlags(&S.done.p, hipEventDisableTiming));
    if (int rc = enqueue_detect(h, P, nframes, FrameSrc{nullptr, 0, d_frames}, channels, kDepth8U)) return rc;
    if (int rc = enqueue_argmin_readback(h, P, nframes, P.d_scales.p, S.cb, h->nms, h->stream)) return rc;
    HIPCHK(h, hipEventRecord(S.done.p, h->stream));
    HIPCHK(h, hipGetLastError());
    h->nsubmitted += 1;
    return PBD_OK;
}

int pbd_detect_batch_submit(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                            size_t stride_bytes)
{
    return entry(h, imgs, kBusyOk, [&]() -> int {
        if (h->nsubmitted - h->nwaited >= 2) return fail(h, PBD_ERR_STATE, "two batches are already in flight: call pbd_detect_batch_wait first");
        Plan *P = nullptr;
        if (int rc = check_detect(h, nframes, FrameSrc{imgs, stride_bytes, nullptr}, rows, cols, channels, kDepth8U, &P)) return rc;
        const size_t row_bytes = (size_t)cols * channels, frame_bytes = row_bytes * rows, bytes = frame_bytes * nframes;
        pbd_handle::Slot &S = h->slot[h->nsubmitted & 1];
        if (!h->stream_copy.s) HIPCHK(h, h->stream_copy.create());
        if (!S.copied.p) HIPCHK(h, hipEventCreateWithFlags(&S.copied.p, hipEventDisableTiming));
        HIPCHK(h, S.pinned.ensure(bytes, bytes + bytes / 8));
        HIPCHK(h, S.frames.ensure(bytes));
        // host staging (this is what overlaps the kernels of the batch submitted before), then one asynchronous copy
        for (int i = 0; i < nframes; ++i) {
            char *dst = S.pinned.as<char>() + (size_t)i * frame_bytes;
            const char *src = static_cast<const char *>(imgs[i]);
            if (stride_bytes == row_bytes) memcpy(dst, src, frame_bytes);
            else for (int y = 0; y < rows; ++y) memcpy(dst + (size_t)y * row_bytes, src + (size_t)y * stride_bytes, row_bytes);
        }
        HIPCHK(h, hipMemcpyAsync(S.frames.p, S.pinned.p, bytes, hipMemcpyHostToDevice, h->stream_copy));
        HIPCHK(h, hipEventRecord(S.copied.p, h->stream_copy));
        HIPCHK(h, hipStreamWaitEvent(h->stream, S.copied.p, 0));
        return submit_enqueue(h, S, *P, nframes, S.frames.p, channels);
    });
}

int pbd_detect_batch_device_submit(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels)
{
    return entry(h, d_frames, kBusyOk, [&]() -> int {
        if (h->nsubmitted - h->nwaited >= 2) return fail(h, PBD_ERR_STATE, "two batches are already in flight: call pbd_detect_batch_wait first");
        Plan *P = nullptr;
        if (int rc = check_detect(h, nframes, FrameSrc{nullptr, 0, d_frames}, rows, cols, channels, kDepth8U, &P)) return rc;
        return submit_enqueue(h, h->slot[h->nsubmitted & 1], *P, nframes, d_frames, channels);
    });
}

int pbd_detect_batch_wait(pbd_handle *h, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, cand && ncand, kBusyOk, [&]() -> int {
        if (h->nsubmitted == h->nwaited) return fail(h, PBD_ERR_STATE, "no batch in flight");
        pbd_handle::Slot &S = h->slot[h->nwaited & 1];
        h->nwaited += 1;                       // the slot is released whatever happens below
        HIPCHK(h, hipEventSynchronize(S.done.p));
        if (!h->stream_d2h.s) HIPCHK(h, h->stream_d2h.create());
        // (a list longer than the speculative copy is fetched on a stream of its own: the compute stream may already hold
        //  the next batch, whose kernels this copy must not queue behind -- and they do not touch this slot's payload)
        return argmin_deliver(h, S.cb, h->stream_d2h, cand, capacity, ncand);
    });
}

// Device-resident output (new surface, for multi-GPU jobs and device pipelines): the whole path with the candidate list
// left ON THE DEVICE in the caller's buffer; asynchronous.  See include/pbd.h.
int pbd_detect_batch_device_out(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                                int frame_offset, int32_t *d_payload, int capacity)
{
    return entry(h, d_frames && d_payload, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        const FrameSrc src{nullptr, 0, d_frames};
        Plan *P = nullptr;
        if (int rc = check_detect(h, nframes, src, rows, cols, channels, kDepth8U, &P)) return rc;
        if (int rc = enqueue_detect(h, *P, nframes, src, channels, kDepth8U)) return rc;
        if (int rc = enqueue_argmin_out(h, *P, nframes, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

int pbd_argmin_device_out(pbd_handle *h, int frame_offset, int32_t *d_payload, int capacity)
{
    return entry(h, d_payload, kIdle, [&]() -> int {
        const Resident &r = h->res;
        if (!r.plan || !r.dp || (r.plan->kind != 0 && r.plan->kind != 2)) return fail(h, PBD_ERR_STATE, "no detect result is resident on the device");
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = enqueue_argmin_out(h, *r.plan, r.frames, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

// Candidate::boundingBox3D(im, depth) per record (include/Candidate.hpp:140-216).  See include/pbd.h.
int pbd_boxes3d(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                const int32_t *cand, int ncand, int frame_offset, double *out)
{
    return entry(h, depth && im_rows && im_cols && (ncand <= 0 || (cand && out)), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_boxes3d_frames(h, nframes, depth, depth_code, im_rows, im_cols, true)) return rc;
        if (int rc = check_boxes3d_records(h, nframes, cand, ncand, frame_offset)) return rc;
        if (ncand == 0) return PBD_OK;
        HIPCHK(h, h->b3_out.ensure((size_t)ncand * 6 * sizeof(double)));
        std::vector<Box3dFrame> tab;
        if (int rc = upload_boxes3d_host(h, nframes, depth, depth_code, im_rows, im_cols, cand, ncand, tab)) return rc;
        if (int rc = enqueue_boxes3d(h, tab, depth_code, h->b3_rec.as<int32_t>(), ncand, frame_offset, h->b3_out.as<double>())) return rc;
        HIPCHK(h, hipMemcpyAsync(out, h->b3_out.p, (size_t)ncand * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_boxes3d_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, const int *im_rows, const int *im_cols,
                       const int32_t *d_payload, int capacity, int frame_offset, double *d_out)
{
    return entry(h, d_depth && im_rows && im_cols && d_payload && (capacity <= 0 || d_out), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_boxes3d_frames(h, nframes, d_depth, depth_code, im_rows, im_cols, false)) return rc;
        if (capacity == 0) return PBD_OK;
        std::vector<Box3dFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f)
            tab[f] = Box3dFrame{static_cast<const uint8_t *>(d_depth[f].data), d_depth[f].rows, d_depth[f].cols,
                                (long long)d_depth[f].stride_bytes, im_rows[f], im_cols[f]};
        return enqueue_boxes3d(h, tab, depth_code, d_payload, capacity, frame_offset, d_out);
    });
}

// SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-95).  See include/pbd.h.
int pbd_depth_consistency(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, float zfactor, const int32_t *cand, int ncand,
                          int frame_offset, int32_t *out, int capacity, int *nout)
{
    return entry(h, depth && nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (int rc = check_dc_frames(h, nframes, depth, depth_code, zfactor, true)) return rc;
        if (int rc = check_dc_records(h, nframes, cand, ncand, frame_offset)) return rc;
        if (ncand == 0) return PBD_OK;
        // the depth images packed with dense rows (the pbd_boxes3d host form's buffers)
        const std::vector<int> ones(nframes, 1);
        std::vector<Box3dFrame> tab;
        if (int rc = upload_boxes3d_host(h, nframes, depth, depth_code, ones.data(), ones.data(), cand, 0, tab)) return rc;
        return host_list_call(h, h->dc_rec, h->dc_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_dc(h, tab, depth_code, zfactor, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_depth_consistency_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, float zfactor,
                                 const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, d_depth && d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 0 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d, out_capacity %d", capacity, out_capacity);
        if (int rc = check_dc_frames(h, nframes, d_depth, depth_code, zfactor, false)) return rc;
        std::vector<Box3dFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f)
            tab[f] = Box3dFrame{static_cast<const uint8_t *>(d_depth[f].data), d_depth[f].rows, d_depth[f].cols,
                                (long long)d_depth[f].stride_bytes, 0, 0};
        return enqueue_dc(h, tab, depth_code, zfactor, d_payload, capacity, frame_offset, d_out, out_capacity);
    });
}

// Candidate::sort + Candidate::nonMaximaSuppression of a caller's list (the pbd_set_nms stage).  See include/pbd.h.
int pbd_suppress(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap, const int32_t *cand, int ncand,
                 int frame_offset, int32_t *out, int capacity, int *nout)
{
    return entry(h, im_rows && im_cols && nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        Plan *P = nullptr;
        if (int rc = get_suppress_plan(h, nframes, im_rows, im_cols, &P)) return rc;
        const int stride = ::stride(h);
        for (int i = 0; i < ncand; ++i) {
            const int32_t *r = cand + (size_t)i * stride;
            const long long f = (long long)r[0] - frame_offset;
            const long long g = i > 0 ? (long long)cand[(size_t)(i - 1) * stride] - frame_offset : 0;
            if (f < 0 || f >= nframes || f < g)
                return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d outside 0..%d or below the previous record's", i,
                            r[0], frame_offset, nframes - 1);
            if (r[6] < 1 || r[6] > h->max_parts) return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (1..%d)", i, r[6], h->max_parts);
        }
        if (ncand == 0) return PBD_OK;
        return host_list_call(h, h->sup_in, h->sup_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_post(h, nframes, 0, 0, overlap, din, ncand, 0, dout, ncand, h->stream, P, frame_offset);
        });
    });
}

int pbd_suppress_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap, const int32_t *d_payload,
                        int capacity, int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, im_rows && im_cols && d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 1 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d (>= 1), out_capacity %d", capacity, out_capacity);
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        Plan *P = nullptr;
        if (int rc = get_suppress_plan(h, nframes, im_rows, im_cols, &P)) return rc;
        HIPCHK(h, h->sup_bad.ensure(sizeof(int)));
        if (int rc = enqueue_post(h, nframes, 0, 0, overlap, d_payload, capacity, 0, d_out, out_capacity, h->stream, P, frame_offset,
                                  h->sup_bad.as<int>())) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

// PointCloudClusterer::computeBoundingBoxes after boundingBox3D (include/PointCloudClusterer.hpp:53-153).  See include/pbd.h.
int pbd_boxes3d_camera(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                       const pbd_pinhole *cams, int parts_mode, const int32_t *cand, int ncand, int frame_offset, double *box,
                       float *centres, int32_t *ncentres, int32_t *dense)
{
    return entry(h, depth && im_rows && im_cols && cams && (ncand <= 0 || (cand && box && centres && ncentres && dense)), kIdle,
                 [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (depth_code != kDepth32F) return check_camera(h, nframes, depth_code, cams, parts_mode);
        if (int rc = check_boxes3d_frames(h, nframes, depth, depth_code, im_rows, im_cols, true)) return rc;
        if (int rc = check_camera(h, nframes, depth_code, cams, parts_mode)) return rc;
        if (int rc = check_boxes3d_records(h, nframes, cand, ncand, frame_offset)) return rc;
        if (ncand == 0) return PBD_OK;
        const size_t nb = (size_t)ncand * 6 * sizeof(double), nc = (size_t)ncand * h->max_parts * 3 * sizeof(float),
                     ni = (size_t)ncand * sizeof(int32_t);
        HIPCHK(h, h->cam_out.ensure(nb + nc + 2 * ni));
        uint8_t *o = h->cam_out.as<uint8_t>();
        std::vector<Box3dFrame> tab;
        if (int rc = upload_boxes3d_host(h, nframes, depth, depth_code, im_rows, im_cols, cand, ncand, tab)) return rc;
        HIPCHK(h, hipMemsetAsync(o + nb, 0, nc, h->stream));
        if (int rc = enqueue_camera(h, tab, depth_code, cams, parts_mode, h->b3_rec.as<int32_t>(), ncand, frame_offset, (double *)o,
                                    (float *)(o + nb), (int32_t *)(o + nb + nc), (int32_t *)(o + nb + nc + ni))) return rc;
        HIPCHK(h, hipMemcpyAsync(box, o, nb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(centres, o + nb, nc, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(ncentres, o + nb + nc, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(dense, o + nb + nc + ni, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_boxes3d_camera_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, const int *im_rows,
                              const int *im_cols, const pbd_pinhole *cams, int parts_mode, const int32_t *d_payload, int capacity,
                              int frame_offset, double *d_box, float *d_centres, int32_t *d_ncentres, int32_t *d_dense)
{
    return entry(h, d_depth && im_rows && im_cols && cams && d_payload && (capacity <= 0 || (d_box && d_centres && d_ncentres && d_dense)),
                 kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (depth_code != kDepth32F) return check_camera(h, nframes, depth_code, cams, parts_mode);
        if (int rc = check_boxes3d_frames(h, nframes, d_depth, depth_code, im_rows, im_cols, false)) return rc;
        if (int rc = check_camera(h, nframes, depth_code, cams, parts_mode)) return rc;
        if (capacity == 0) return PBD_OK;
        std::vector<Box3dFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f)
            tab[f] = Box3dFrame{static_cast<const uint8_t *>(d_depth[f].data), d_depth[f].rows, d_depth[f].cols,
                                (long long)d_depth[f].stride_bytes, im_rows[f], im_cols[f]};
        return enqueue_camera(h, tab, depth_code, cams, parts_mode, d_payload, capacity, frame_offset, d_box, d_centres, d_ncentres,
                              d_dense);
    });
}

// PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:157-293).  See include/pbd.h.
int pbd_cluster_objects(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const double *boxes, const int *frames, int nboxes,
                        float *centres, int32_t *counts, int32_t *indices, int index_capacity, int *needed)
{
    return entry(h, clouds && needed && (nboxes <= 0 || (boxes && frames && centres && counts)) && (index_capacity <= 0 || indices),
                 kIdle, [&]() -> int {
        *needed = 0;
        if (nboxes < 0 || index_capacity < 0) return fail(h, PBD_ERR_INVALID, "nboxes %d, index capacity %d", nboxes, index_capacity);
        if (int rc = check_clouds(h, nclouds, clouds, true)) return rc;
        for (int i = 0; i < nboxes; ++i)
            if (frames[i] < 0 || frames[i] >= nclouds) return fail(h, PBD_ERR_INVALID, "box %d: frame %d outside 0..%d", i, frames[i], nclouds - 1);
        if (nboxes == 0) return PBD_OK;
        // the clouds' x, y, z, packed
        size_t total = 0;
        for (int f = 0; f < nclouds; ++f) total += (size_t)clouds[f].rows * clouds[f].cols;
        std::vector<float> packed(total * 3);
        std::vector<CloudFrame> tab(nclouds);
        HIPCHK(h, h->cl_cloud.ensure(total * 12 + 16));
        size_t off = 0;
        for (int f = 0; f < nclouds; ++f) {
            const pbd_cloud &c = clouds[f];
            for (int r = 0; r < c.rows; ++r)
                for (int k = 0; k < c.cols; ++k)
                    memcpy(&packed[(off + (size_t)r * c.cols + k) * 3],
                           static_cast<const uint8_t *>(c.data) + r * c.row_stride + k * c.point_stride, 12);
            tab[f] = CloudFrame{h->cl_cloud.as<uint8_t>() + off * 12, c.rows, c.cols, 12, (long long)c.cols * 12};
            off += (size_t)c.rows * c.cols;
        }
        HIPCHK(h, hipMemcpyAsync(h->cl_cloud.p, packed.data(), total * 12, hipMemcpyHostToDevice, h->stream));
        // the boxes and a payload of stride 1 holding the frames
        const size_t bb = (size_t)nboxes * 6 * sizeof(double), pb = ((size_t)nboxes + 1) * sizeof(int32_t);
        HIPCHK(h, h->cl_in.ensure(bb + pb + 16));
        std::vector<int32_t> pay(nboxes + 1);
        pay[0] = nboxes;
        for (int i = 0; i < nboxes; ++i) pay[i + 1] = frames[i];
        HIPCHK(h, hipMemcpyAsync(h->cl_in.p, boxes, bb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->cl_in.as<uint8_t>() + bb, pay.data(), pb, hipMemcpyHostToDevice, h->stream));
        const double *d_boxes = h->cl_in.as<double>();
        const int32_t *d_pay = reinterpret_cast<const int32_t *>(h->cl_in.as<uint8_t>() + bb);
        // outputs: centres, counts, status, then the indices (at most the cropped points)
        long long crop_cap = std::max<long long>(h->cl_crop_cap, 1 << 16);
        long long status[2] = {0, 0};
        for (int pass = 0; pass < 2; ++pass) {
            const size_t oc = (size_t)nboxes * 12, on = (size_t)nboxes * 4;
            HIPCHK(h, h->cl_out.ensure(oc + on + 16 + 16 + (size_t)crop_cap * 4));
            uint8_t *o = h->cl_out.as<uint8_t>();
            long long *d_status = reinterpret_cast<long long *>(o + (oc + on + 15) / 16 * 16);
            int32_t *d_idx = reinterpret_cast<int32_t *>(d_status + 2);
            if (int rc = enqueue_cluster(h, tab, d_pay, nboxes, 1, 0, d_boxes, (int)crop_cap, (int)crop_cap, (float *)o,
                                         (int32_t *)(o + oc), d_idx, d_status)) return rc;
            HIPCHK(h, hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (status[0] <= crop_cap) {
                h->cl_crop_cap = std::max(h->cl_crop_cap, crop_cap);
                if (status[1] > index_capacity) {
                    *needed = (int)status[1];
                    return fail(h, PBD_ERR_CAPACITY, "the kept clusters hold %lld indices, capacity %d", status[1], index_capacity);
                }
                *needed = (int)status[1];
                HIPCHK(h, hipMemcpyAsync(centres, o, oc, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipMemcpyAsync(counts, o + oc, on, hipMemcpyDeviceToHost, h->stream));
                if (status[1] > 0) HIPCHK(h, hipMemcpyAsync(indices, d_idx, (size_t)status[1] * 4, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                return PBD_OK;
            }
            if (status[0] > kClMaxCrop) return fail(h, PBD_ERR_INVALID, "%lld cropped points (at most 2^29)", status[0]);
            crop_cap = status[0];                      // the first pass counted them all: the second fits
        }
        return fail(h, PBD_ERR_HIP, "cropped points changed between two passes");
    });
}

int pbd_cluster_objects_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const int32_t *d_payload, int capacity,
                               int frame_offset, const double *d_boxes, int crop_capacity, int index_capacity, float *d_centres,
                               int32_t *d_counts, int32_t *d_indices, long long *d_status)
{
    return entry(h, d_clouds && d_payload && d_status && (capacity <= 0 || (d_boxes && d_centres && d_counts)) &&
                    (index_capacity <= 0 || d_indices), kIdle, [&]() -> int {
        if (capacity < 0 || crop_capacity < 0 || index_capacity < 0 || crop_capacity > kClMaxCrop)
            return fail(h, PBD_ERR_INVALID, "capacity %d, crop capacity %d (at most 2^29), index capacity %d", capacity, crop_capacity,
                        index_capacity);
        if (int rc = check_clouds(h, nclouds, d_clouds, false)) return rc;
        if (capacity == 0) {
            HIPCHK(h, hipMemsetAsync(d_status, 0, 2 * sizeof(long long), h->stream));
            return PBD_OK;
        }
        std::vector<CloudFrame> tab(nclouds);
        for (int f = 0; f < nclouds; ++f)
            tab[f] = CloudFrame{static_cast<const uint8_t *>(d_clouds[f].data), d_clouds[f].rows, d_clouds[f].cols,
                                (long long)d_clouds[f].point_stride, (long long)d_clouds[f].row_stride};
        return enqueue_cluster(h, tab, d_payload, capacity, stride(h), frame_offset, d_boxes, crop_capacity, index_capacity, d_centres,
                               d_counts, d_indices, d_status);
    });
}

// PointCloudClusterer::organizedMultiplaneSegmentation (include/PointCloudClusterer.hpp:294-336).  See include/pbd.h.
int pbd_remove_planes(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const pbd_plane_params *params, float *points, int32_t *kept,
                      int32_t *nkept, int32_t *labels, float *planes, int32_t *inliers, int32_t *nplanes, int plane_capacity, int *needed)
{
    return entry(h, clouds && points && kept && nkept && labels && nplanes && needed && (plane_capacity <= 0 || (planes && inliers)),
                 kIdle, [&]() -> int {
        *needed = 0;
        const pbd_plane_params q = params ? *params : plane_defaults();
        if (plane_capacity < 0) return fail(h, PBD_ERR_INVALID, "plane capacity %d", plane_capacity);
        if (int rc = check_plane_params(h, q)) return rc;
        if (int rc = check_organized(h, nclouds, clouds, true)) return rc;
        // the clouds' x, y, z, packed
        std::vector<pbd_cloud> packed_desc(nclouds);
        size_t total = 0;
        for (int f = 0; f < nclouds; ++f) total += (size_t)clouds[f].rows * clouds[f].cols;
        std::vector<float> packed(total * 3);
        HIPCHK(h, h->pl_cloud.ensure(total * 12 + 16));
        size_t off = 0;
        for (int f = 0; f < nclouds; ++f) {
            const pbd_cloud &c = clouds[f];
            for (int r = 0; r < c.rows; ++r)
                for (int k = 0; k < c.cols; ++k)
                    memcpy(&packed[(off + (size_t)r * c.cols + k) * 3],
                           static_cast<const uint8_t *>(c.data) + r * c.row_stride + k * c.point_stride, 12);
            packed_desc[f] = pbd_cloud{h->pl_cloud.as<uint8_t>() + off * 12, c.rows, c.cols, 12, (size_t)c.cols * 12};
            off += (size_t)c.rows * c.cols;
        }
        HIPCHK(h, hipMemcpyAsync(h->pl_cloud.p, packed.data(), total * 12, hipMemcpyHostToDevice, h->stream));
        // outputs: status, counts, then points, kept, labels, planes, inliers
        const size_t cap = (size_t)std::max(plane_capacity, 0);
        const size_t o_stat = 0, o_nk = 16, o_np = o_nk + (size_t)nclouds * 4, o_pts = (o_np + (size_t)nclouds * 4 + 15) / 16 * 16,
                     o_kept = o_pts + total * 12, o_lab = o_kept + total * 4, o_pl = (o_lab + total * 4 + 15) / 16 * 16,
                     o_in = o_pl + (size_t)nclouds * cap * 16, o_end = o_in + (size_t)nclouds * cap * 4;
        HIPCHK(h, h->pl_out.ensure(o_end + 16));
        uint8_t *o = h->pl_out.as<uint8_t>();
        if (int rc = enqueue_planes(h, plane_table(nclouds, packed_desc.data()), q, (float *)(o + o_pts), (int32_t *)(o + o_kept),
                                    (int32_t *)(o + o_nk), (int32_t *)(o + o_lab), (float *)(o + o_pl), (int32_t *)(o + o_in),
                                    (int32_t *)(o + o_np), (int)cap, (long long *)(o + o_stat))) return rc;
        long long status[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(status, o + o_stat, sizeof status, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *needed = (int)status[1];
        if (status[1] > plane_capacity)
            return fail(h, PBD_ERR_CAPACITY, "a cloud holds %lld planes, capacity %d", status[1], plane_capacity);
        HIPCHK(h, hipMemcpyAsync(nkept, o + o_nk, (size_t)nclouds * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(nplanes, o + o_np, (size_t)nclouds * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(points, o + o_pts, total * 12, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(kept, o + o_kept, total * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(labels, o + o_lab, total * 4, hipMemcpyDeviceToHost, h->stream));
        if (cap) {
            HIPCHK(h, hipMemcpyAsync(planes, o + o_pl, (size_t)nclouds * cap * 16, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(inliers, o + o_in, (size_t)nclouds * cap * 4, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_remove_planes_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const pbd_plane_params *params, float *d_points,
                             int32_t *d_kept, int32_t *d_nkept, int32_t *d_labels, float *d_planes, int32_t *d_inliers,
                             int32_t *d_nplanes, int plane_capacity, long long *d_status)
{
    return entry(h, d_clouds && d_points && d_kept && d_nkept && d_labels && d_nplanes && d_status &&
                    (plane_capacity <= 0 || (d_planes && d_inliers)), kIdle, [&]() -> int {
        const pbd_plane_params q = params ? *params : plane_defaults();
        if (plane_capacity < 0) return fail(h, PBD_ERR_INVALID, "plane capacity %d", plane_capacity);
        if (int rc = check_plane_params(h, q)) return rc;
        if (int rc = check_organized(h, nclouds, d_clouds, false)) return rc;
        return enqueue_planes(h, plane_table(nclouds, d_clouds), q, d_points, d_kept, d_nkept, d_labels, d_planes, d_inliers, d_nplanes,
                              plane_capacity, d_status);
    });
}

// Mixed-size calls (new surface): nframes frames of any sizes, planned as one virtual frame.  See include/pbd.h.
int pbd_detect_frames(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int32_t *cand, int capacity,
                      int *ncand)
{
    return entry(h, frames && cand && ncand, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, true, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, true)) return rc;
        return run_argmin(h, *P, 1, P->d_scales.p, h->nms, cand, capacity, ncand);
    });
}

int pbd_detect_frames_device(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int32_t *cand,
                             int capacity, int *ncand)
{
    return entry(h, frames && cand && ncand, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, false, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, false)) return rc;
        return run_argmin(h, *P, 1, P->d_scales.p, h->nms, cand, capacity, ncand);
    });
}

int pbd_detect_frames_device_out(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int frame_offset,
                                 int32_t *d_payload, int capacity)
{
    return entry(h, frames && d_payload, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        Plan *P = nullptr;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, false, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, false)) return rc;
        if (int rc = enqueue_argmin_out(h, *P, 1, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

void *pbd_stream(const pbd_handle *h) { return h ? reinterpret_cast<void *>(h->stream.s) : nullptr; }

int pbd_get_stage(pbd_handle *h, int stage, int frame, int level, void *dst, size_t dst_bytes)
{
    return entry(h, dst, kIdle, [&]() -> int {
        const Resident &r = h->res;
        if (!r.plan) return fail(h, PBD_ERR_STATE, "nothing has been computed");
        const Plan &P = *r.plan;
        if (!resident_level(r, frame, level, &frame, &level)) return fail(h, PBD_ERR_INVALID, "frame/level out of range");
        const LevelDesc &d = P.lv[level];
        const size_t hw = (size_t)d.rows * d.cols, cell = (size_t)frame * P.cell_per_frame + d.cell_off;
        const void *src = nullptr;
        size_t bytes = 0;
        switch (stage) {
        case PBD_STAGE_FEATURES:
            if (!r.features) return fail(h, PBD_ERR_STATE, "features not computed");
            src = h->feat.as<char>() + cell * 32 * h->rs; bytes = hw * 32 * h->rs; break;
        case PBD_STAGE_RESPONSES:
            if (!r.resp) return fail(h, PBD_ERR_STATE, "responses not computed");
            src = h->resp.as<char>() + cell * h->F * h->resp_es; bytes = hw * h->F * h->rs; break;
        case PBD_STAGE_ROOTV:
            if (!r.dp) return fail(h, PBD_ERR_STATE, "dp not computed");
            src = h->rootv.as<char>() + cell * h->NC * h->rs; bytes = hw * h->NC * h->rs; break;
        case PBD_STAGE_ROOTI:
            if (!r.dp) return fail(h, PBD_ERR_STATE, "dp not computed");
            src = h->rooti.as<int>() + cell * h->NC; bytes = hw * h->NC * sizeof(int); break;
        default: return fail(h, PBD_ERR_INVALID, "unknown stage %d", stage);
        }
        if (dst_bytes < bytes) return fail(h, PBD_ERR_INVALID, "destination holds %zu bytes, need %zu", dst_bytes, bytes);
        if (stage == PBD_STAGE_RESPONSES) {
            if (int rc = read_responses(h, dst, src, hw * h->F)) return rc;
        } else if (bytes) {
            HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

// Candidate::mask (include/Candidate.hpp:306-331) and rgb & (mask != 0) (ros/Messages.cpp:157-174).  See include/pbd.h.
int pbd_candidate_mask(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *cand, int ncand, int frame_offset,
                       uint8_t *const *labels, const size_t *label_pitch, int channels, const uint8_t *const *colour,
                       const size_t *colour_pitch, uint8_t *const *masked, const size_t *masked_pitch)
{
    return entry(h, im_rows && im_cols && (ncand <= 0 || cand), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_mask_frames(h, nframes, im_rows, im_cols, labels, label_pitch, channels, colour, colour_pitch, masked,
                                       masked_pitch)) return rc;
        const int stride = ::stride(h);
        for (int i = 0; i < ncand; ++i) {
            const int32_t *r = cand + (size_t)i * stride;
            const long long f = (long long)r[0] - frame_offset;
            const long long g = i > 0 ? (long long)cand[(size_t)(i - 1) * stride] - frame_offset : 0;
            if (f < 0 || f >= nframes || f < g)
                return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d outside 0..%d or below the previous record's", i,
                            r[0], frame_offset, nframes - 1);
            if (r[6] < 1 || r[6] > h->max_parts) return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (1..%d)", i, r[6], h->max_parts);
        }
        if (!labels && !masked) return PBD_OK;
        const int cn = masked ? channels : 0;
        // the records as a payload, each frame's labels and colour packed with dense rows in the handle's own buffers
        size_t lab_total = 0, img_total = 0;
        for (int f = 0; f < nframes; ++f) {
            lab_total += labels ? (size_t)im_rows[f] * im_cols[f] : 0;
            img_total += (size_t)im_rows[f] * im_cols[f] * cn;
        }
        const size_t lab_bytes = (lab_total + 255) / 256 * 256;
        HIPCHK(h, h->mk_img.ensure(lab_bytes + img_total + 256));
        HIPCHK(h, h->mk_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, hipMemcpyAsync(h->mk_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        if (ncand) HIPCHK(h, hipMemcpyAsync(h->mk_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t),
                                            hipMemcpyHostToDevice, h->stream));
        std::vector<MaskFrame> tab(nframes);
        uint8_t *lab = h->mk_img.as<uint8_t>(), *img = lab + lab_bytes;
        for (int f = 0; f < nframes; ++f) {
            const size_t lrow = (size_t)im_cols[f], crow = lrow * cn;
            MaskFrame &fr = tab[f];
            fr = MaskFrame{};
            fr.rows = im_rows[f]; fr.cols = im_cols[f];
            if (labels) { fr.labels = lab; fr.label_pitch = (long long)lrow; lab += lrow * im_rows[f]; }
            if (masked) {
                HIPCHK(h, hipMemcpy2DAsync(img, crow, colour[f], colour_pitch[f], crow, im_rows[f], hipMemcpyHostToDevice, h->stream));
                fr.colour = img; fr.masked = img; fr.colour_pitch = fr.masked_pitch = (long long)crow;
                img += crow * im_rows[f];
            }
        }
        if (int rc = enqueue_mask(h, tab, cn, h->mk_rec.as<int32_t>(), ncand, frame_offset, nullptr)) return rc;
        for (int f = 0; f < nframes; ++f) {
            if (labels)
                HIPCHK(h, hipMemcpy2DAsync(labels[f], label_pitch[f], tab[f].labels, (size_t)im_cols[f], (size_t)im_cols[f], im_rows[f],
                                           hipMemcpyDeviceToHost, h->stream));
            if (masked) {
                const size_t crow = (size_t)im_cols[f] * cn;
                HIPCHK(h, hipMemcpy2DAsync(masked[f], masked_pitch[f], tab[f].masked, crow, crow, im_rows[f], hipMemcpyDeviceToHost,
                                           h->stream));
            }
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_candidate_mask_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *d_payload, int capacity,
                              int frame_offset, uint8_t *const *d_labels, const size_t *label_pitch, int channels,
                              const uint8_t *const *d_colour, const size_t *colour_pitch, uint8_t *const *d_masked,
                              const size_t *masked_pitch, int32_t *d_status)
{
    return entry(h, im_rows && im_cols && d_payload && d_status, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_mask_frames(h, nframes, im_rows, im_cols, d_labels, label_pitch, channels, d_colour, colour_pitch, d_masked,
                                       masked_pitch)) return rc;
        std::vector<MaskFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f) {
            MaskFrame &fr = tab[f];
            fr = MaskFrame{};
            fr.rows = im_rows[f]; fr.cols = im_cols[f];
            if (d_labels) { fr.labels = d_labels[f]; fr.label_pitch = (long long)label_pitch[f]; }
            if (d_masked) {
                fr.colour = d_colour[f]; fr.masked = d_masked[f];
                fr.colour_pitch = (long long)colour_pitch[f]; fr.masked_pitch = (long long)masked_pitch[f];
            }
        }
        return enqueue_mask(h, tab, d_masked ? channels : 0, d_payload, capacity, frame_offset, d_status);
    });
}

// PartsBasedDetectorNode::messagePoses (ros/Messages.cpp:187-234) per record.  See include/pbd.h.
int pbd_part_poses(pbd_handle *h, int n, const float *centres, const int32_t *ncentres, const int32_t *dense, int32_t *count,
                   float *position, float *orientation, float *eigenvalues)
{
    return entry(h, n <= 0 || (centres && ncentres && dense && count && position && orientation && eigenvalues), kIdle, [&]() -> int {
        if (n < 0) return fail(h, PBD_ERR_INVALID, "n %d", n);
        for (int i = 0; i < n; ++i)
            if (ncentres[i] < 0 || ncentres[i] > h->max_parts)
                return fail(h, PBD_ERR_INVALID, "record %d: ncentres %d (0..%d)", i, ncentres[i], h->max_parts);
        if (n == 0) return PBD_OK;
        const size_t nc = (size_t)n * h->max_parts * 3 * sizeof(float), ni = (size_t)n * sizeof(int32_t), n3 = (size_t)n * 3 * sizeof(float),
                     n4 = (size_t)n * 4 * sizeof(float);
        HIPCHK(h, h->ps_buf.ensure(nc + 3 * ni + 2 * n3 + n4 + 256));
        uint8_t *b = h->ps_buf.as<uint8_t>();
        float *d_cen = (float *)b, *d_pos = (float *)(b + nc), *d_ori = (float *)(b + nc + n3), *d_ev = (float *)(b + nc + n3 + n4);
        int32_t *d_nc = (int32_t *)(b + nc + 2 * n3 + n4), *d_dn = d_nc + n, *d_cnt = d_dn + n, *d_word = d_cnt + n;
        HIPCHK(h, hipMemcpyAsync(d_word, &n, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_cen, centres, nc, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_nc, ncentres, ni, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dn, dense, ni, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_poses(h, d_word, n, d_cen, d_nc, d_dn, d_cnt, d_pos, d_ori, d_ev)) return rc;
        HIPCHK(h, hipMemcpyAsync(count, d_cnt, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(position, d_pos, n3, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(orientation, d_ori, n4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(eigenvalues, d_ev, n3, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_part_poses_device(pbd_handle *h, const int32_t *d_payload, int capacity, const float *d_centres, const int32_t *d_ncentres,
                          const int32_t *d_dense, int32_t *d_count, float *d_position, float *d_orientation, float *d_eigenvalues)
{
    return entry(h, d_payload && (capacity <= 0 || (d_centres && d_ncentres && d_dense && d_count && d_position && d_orientation &&
                                                    d_eigenvalues)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (capacity == 0) return PBD_OK;
        return enqueue_poses(h, d_payload, capacity, d_centres, d_ncentres, d_dense, d_count, d_position, d_orientation, d_eigenvalues);
    });
}

// Training examples (matlab/detection/detect.m backtrack + qp_write).  See include/pbd.h.
int pbd_model_vector_len(const pbd_handle *h) { return h ? (int)(h->mvec.size() / h->rs) : 0; }

int pbd_model_vector(pbd_handle *h, void *w)
{
    return entry(h, w, kBusyOk, [&]() -> int {
        memcpy(w, h->mvec.data(), h->mvec.size());
        return PBD_OK;
    });
}

int pbd_example_stride(const pbd_handle *h, int *hdr_words, int *values)
{
    if (!h || !hdr_words || !values) return PBD_ERR_INVALID;
    *hdr_words = h->ex_hdr_words;
    *values = h->ex_values;
    return PBD_OK;
}

int pbd_examples(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, int32_t *hdr, void *values)
{
    return entry(h, ncand <= 0 || (cand && hdr && values), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_examples_state(h)) return rc;
        const int stride = ::stride(h);
        const Resident &res = resident_owner(h)->res;
        const Plan &P = *res.plan;
        for (int i = 0; i < ncand; ++i) {
            const int32_t *r = cand + (size_t)i * stride;
            const long long f = (long long)r[0] - frame_offset;
            int bf = 0, bl = 0;
            if (f < INT32_MIN || f > INT32_MAX || !resident_level(res, (int)f, r[2], &bf, &bl))
                return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d / level %d outside the resident result", i, r[0],
                            frame_offset, r[2]);
            const LevelDesc &d = P.lv[bl];
            if (r[1] < 0 || r[1] >= h->NC) return fail(h, PBD_ERR_INVALID, "record %d: component %d (0..%d)", i, r[1], h->NC - 1);
            if (r[3] < 0 || r[3] >= d.cols || r[4] < 0 || r[4] >= d.rows)
                return fail(h, PBD_ERR_INVALID, "record %d: root (%d, %d) outside the %d x %d map of level %d%s", i, r[3], r[4], d.cols,
                            d.rows, r[2], d.rows ? "" : " (a level of another rank)");
        }
        if (ncand == 0) return PBD_OK;
        const size_t hb = (size_t)ncand * h->ex_hdr_words * sizeof(int32_t), vb = (size_t)ncand * h->ex_values * h->rs;
        const size_t hb_al = (hb + 255) / 256 * 256;
        HIPCHK(h, h->ex_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, h->ex_out.ensure(hb_al + vb));
        HIPCHK(h, hipMemcpyAsync(h->ex_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->ex_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                                 h->stream));
        int32_t *d_hdr = h->ex_out.as<int32_t>();
        char *d_val = h->ex_out.as<char>() + hb_al;
        if (int rc = enqueue_examples(h, h->ex_rec.as<int32_t>(), ncand, frame_offset, d_hdr, d_val)) return rc;
        HIPCHK(h, hipMemcpyAsync(hdr, d_hdr, hb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(values, d_val, vb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

// Latent positives (matlab/detection/detect.m with a bbox: testoverlap masks, bbox.m fixed mixtures).  See include/pbd.h.
int pbd_detect_latent(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, const int32_t *boxes,
                      const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found)
{
    return entry(h, frames && boxes && cand && found, kIdle, [&]() -> int {
        if (h->shard_world > 1)
            return fail(h, PBD_ERR_UNSUPPORTED, "latent detection with level sharding (world %d): the best root is over every level",
                        h->shard_world);
        const int nparts = h->part_offset[1] - h->part_offset[0];
        for (int c = 1; c < h->NC; ++c)
            if (h->part_offset[c + 1] - h->part_offset[c] != nparts)
                return fail(h, PBD_ERR_UNSUPPORTED, "latent detection needs one part count in every component (component %d has %d, "
                            "component 0 %d)", c, h->part_offset[c + 1] - h->part_offset[c], nparts);
        if (h->resp_half) return fail(h, PBD_ERR_UNSUPPORTED, "latent detection in PBD_CONV_MFMA_F16: -1e10 has no fp16 value");
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        if (int rc = check_bank(h)) return rc;
        if (h->filter_ksize != h->model_ksize) return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's");
        if (!h->lat) {   // the latent twin: the same model with one filter per (component, part, mixture), on this handle's stream
            const int T = h->totmix;
            std::vector<int> ks(T), fid(T);
            std::vector<int64_t> off(T);
            for (int gm = 0; gm < T; ++gm) {
                fid[gm] = gm;
                ks[gm] = h->model_ksize[h->filterid[gm]];
                off[gm] = h->model_foff[h->filterid[gm]];
            }
            const size_t fbase = (size_t)h->nbias + 4 * (size_t)h->ndefs;
            pbd_model m{};
            m.ncomponents = h->NC; m.nfilters = T; m.flen = 32; m.filter_ksize = ks.data(); m.filter_offset = off.data();
            if (h->f64) m.filters_f64 = reinterpret_cast<const double *>(h->mvec.data()) + fbase;
            else m.filters_f32 = reinterpret_cast<const float *>(h->mvec.data()) + fbase;
            m.nbias = h->nbias; m.biasw = h->biasw.data(); m.ndefs = h->ndefs; m.defw = h->defw.data(); m.anchors = h->anchors.data();
            m.part_offset = h->part_offset.data(); m.parentid = h->parentid.data(); m.mix_offset = h->mix_offset.data();
            m.filterid = fid.data(); m.biasid = h->biasid.data(); m.defid = h->defid.data();
            m.thresh = h->thresh; m.sbin = h->sbin; m.interval = h->interval; m.norient = h->norient;
            pbd_config cfg = h->cfg;
            cfg.max_candidates = std::max(cfg.max_batch, 1);
            cfg.stream = reinterpret_cast<void *>(h->stream.s);
            pbd_handle *t = nullptr;
            if (int rc = pbd_create(&m, &cfg, &t)) return fail(h, rc, "latent twin: %s", pbd_last_error(nullptr));
            h->lat.reset(t);
            std::vector<int4> gm(T);
            for (int c = 0; c < h->NC; ++c)
                for (int gp = h->part_offset[c]; gp < h->part_offset[c + 1]; ++gp)
                    for (int g = h->mix_offset[gp]; g < h->mix_offset[gp + 1]; ++g)
                        gm[g] = make_int4(gp - h->part_offset[c], g - h->mix_offset[gp], ks[g], 0);
            HIPCHK(h, h->lat_gm.upload(gm));
        }
        pbd_handle *t = h->lat.get();
        Plan *P = nullptr;
        if (int rc = check_frames_mixed(t, nframes, frames, channels, depth_code, true, &P)) return fail(h, rc, "%s", t->err.c_str());
        const size_t nb = (size_t)nframes * nparts;
        HIPCHK(h, h->lat_in.ensure(nb * sizeof(int4) + nb * sizeof(int) + 64));
        HIPCHK(h, hipMemcpyAsync(h->lat_in.p, boxes, nb * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        int *d_mix = reinterpret_cast<int *>(h->lat_in.as<char>() + nb * sizeof(int4));
        if (mixtures) HIPCHK(h, hipMemcpyAsync(d_mix, mixtures, nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!P->d_frame_lv0.p) HIPCHK(h, P->d_frame_lv0.upload(P->frame_lv0));
        const int stride = ::stride(h);
        HIPCHK(h, h->lat_pay.ensure(((size_t)nframes * stride + 1) * sizeof(int32_t)));
        h->res = Resident{};
        h->res.latent = true;
        LatentParams lp{};
        lp.gmtab = h->lat_gm.p; lp.boxes = h->lat_in.as<int4>(); lp.mix = mixtures ? d_mix : nullptr; lp.nparts = nparts;
        lp.overlap = (double)overlap;
        if (int rc = enqueue_detect_mixed(t, *P, nframes, frames, channels, depth_code, true, &lp)) return fail(h, rc, "%s", t->err.c_str());
        lp.rootv = t->rootv.p; lp.rooti = t->rooti.as<int>(); lp.lv = P->d_lv.p; lp.nlevels = P->nlevels;
        lp.cell_per_frame = P->cell_per_frame; lp.frame_lv0 = P->d_frame_lv0.p; lp.nframes = nframes; lp.NC = h->NC;
        lp.stride = stride; lp.payload = h->lat_pay.as<int32_t>();
        launch_latent_best(lp, h->f64, h->stream);
        if (int rc = enqueue_argmin(t, *P, 1, P->d_scales.p, 0, lp.payload, nframes, h->stream, true)) return fail(h, rc, "%s", t->err.c_str());
        HIPCHK(h, hipMemcpyAsync(cand, lp.payload + 1, (size_t)nframes * stride * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        for (int f = 0; f < nframes; ++f) {
            float sc;
            memcpy(&sc, &cand[(size_t)f * stride + 5], sizeof sc);
            found[f] = sc > -5e9f ? 1 : 0;
        }
        return PBD_OK;
    });
}

int pbd_examples_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_hdr, void *d_values)
{
    return entry(h, d_payload && (capacity <= 0 || (d_hdr && d_values)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_examples_state(h)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_examples(h, d_payload, capacity, frame_offset, d_hdr, d_values);
    });
}

int pbd_profile_enable(pbd_handle *h, int on)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        h->prof.flush();
        h->prof.on = on == 2 ? 2 : (on != 0 ? 1 : 0);
        return PBD_OK;
    });
}
int pbd_profile_reset(pbd_handle *h)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        h->prof.flush();
        for (int k = 0; k < PBD_K_COUNT; ++k) { h->prof.total[k] = 0; h->prof.launches[k] = 0; }
        return PBD_OK;
    });
}
int pbd_profile_read(pbd_handle *h, int k, double *total_ms, int *launches)
{
    return entry(h, k >= 0 && k < PBD_K_COUNT, kBusyOk, [&]() -> int {
        h->prof.flush();
        if (total_ms) *total_ms = h->prof.total[k];
        if (launches) *launches = h->prof.launches[k];
        return PBD_OK;
    });
}
const char *pbd_kernel_name(int k)
{
    static const char *names[PBD_K_COUNT] = {"k_resize", "k_pyrdown", "k_hog_hist", "k_hog_feat", "k_conv", "k_dt_rows",
                                             "k_dt_cols", "k_dp_combine", "k_dp_root", "k_argmin", "k_camera_boxes",
                                             "k_cl_crop_count", "k_cl_crop_scan", "k_cl_crop_scatter", "k_cl_clear", "k_cl_grid_count",
                                             "k_cl_grid_scan", "k_cl_grid_scatter", "k_cl_hook", "k_cl_label", "k_cl_best", "k_cl_select",
                                             "k_cl_out", "k_dc_classify", "k_dc_select", "k_dc_compact", "k_mk_hull", "k_mk_tile",
                                             "k_part_poses", "k_ex_walk", "k_ex_gather", "k_qp_write", "k_qp_score",
                                             "k_qp_pass", "k_qp_lincomb", "k_qp_slots", "k_qp_norm", "k_qp_wraw",
                                             "k_qp_gather"};
    return (k >= 0 && k < PBD_K_COUNT) ? names[k] : "?";
}
int pbd_synchronize(pbd_handle *h)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

}  // extern "C"

// ================================================================================================
// The training QP (matlab/learning/qp_*.m).  See include/pbd.h and DESIGN.md section 6i.  The kernels are in
// pbd_kernels_qp.hip; the host keeps the ids, block tables and b of the entries (for the grouping, the refresh's entry lists
// and l) and orders every call; all per-value work is on the device.
struct pbd_qp {
    std::string err;
    int device = 0;
    Stream stream;
    int cap = 0, L = 0, V = 0, HW = 0, MB = 0, in_hw = 0;
    uint64_t fp = 0;
    double Cpos = 0, Cneg = 0;
    DevBuf x, bm, hd, ids, b, d, a, sv, w, wraw, misc, stage, work, lc, scratch;
    DevTable<double> wreg, w0;
    DevTable<int> noneg, slot_of, slot_len;
    std::vector<double> wreg_h, w0_h;
    std::vector<int> slot_of_h, slot_len_h, slot_off_h;   // coordinate -> layout block; its length and offset
    std::vector<int32_t> h_ids, h_hd;   // [n * 5], [n * HW]
    std::vector<double> h_b;
    int n = 0, nfix = 0, nnoneg = 0;
    double lb = NAN, ub = NAN, loss = 0, l = 0, ww = 0;
    bool have_lb = false;
    int lb_dropped = 0, passes = 0, converged = 0;
};

namespace {

constexpr size_t kQpPruneChunkBytes = size_t(256) << 20;   // prune's scratch: at most this much (or one entry) ...
constexpr int kQpPruneChunkEntries = 256;                  // ... and at most this many entries per chunk

int qp_fail(pbd_qp *q, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try {
        if (q) q->err = buf; else g_create_error = buf;
    } catch (...) {
    }
    return code;
}

#define QPCHK(q, expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (void)hipGetLastError();                                                                \
            return qp_fail(q, e_ == hipErrorOutOfMemory ? PBD_ERR_NOMEM : PBD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                           hipGetErrorString(e_), __FILE__, __LINE__);                              \
        }                                                                                           \
    } while (0)

template <class F>
int qp_entry(pbd_qp *q, bool args_ok, F &&body) noexcept
{
    try {
        if (!q || !args_ok) return PBD_ERR_INVALID;
        (void)hipSetDevice(q->device);
        return body();
    } catch (const std::bad_alloc &) {
        return qp_fail(q, PBD_ERR_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return qp_fail(q, PBD_ERR_INVALID, "unexpected exception: %s", e.what());
    } catch (...) {
        return qp_fail(q, PBD_ERR_INVALID, "unexpected exception");
    }
}

hipError_t qp_alloc(DevBuf &buf, size_t bytes)
{
    buf = DevBuf{};
    const hipError_t e = hipMalloc(&buf.p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess) buf.size = std::max<size_t>(bytes, 16);
    return e;
}

// the model-vector layout of a handle: every bias, deformation and filter block (offset, length), the example strides, and
// its FNV-1a fingerprint
struct QpLayout {
    int L = 0, V = 0, in_hw = 0;
    std::vector<std::pair<int, int> > blocks;
    uint64_t fp = 0;
};
QpLayout qp_layout(const pbd_handle *h)
{
    QpLayout lay;
    lay.L = (int)(h->mvec.size() / h->rs);
    lay.V = h->ex_values;
    lay.in_hw = h->ex_hdr_words;
    for (int b = 0; b < h->nbias; ++b) lay.blocks.push_back({b, 1});
    for (int d = 0; d < h->ndefs; ++d) lay.blocks.push_back({h->nbias + 4 * d, 4});
    const long long fbase = (long long)h->nbias + 4LL * h->ndefs;
    for (size_t f = 0; f < h->model_foff.size(); ++f)
        lay.blocks.push_back({(int)(fbase + h->model_foff[f]), h->model_ksize[f] * h->model_ksize[f] * 32});
    uint64_t v = 1469598103934665603ULL;
    auto mix = [&](long long x) { for (int k = 0; k < 8; ++k) { v ^= (uint64_t)((x >> (8 * k)) & 0xff); v *= 1099511628211ULL; } };
    mix(lay.L); mix(lay.V); mix(lay.in_hw); mix((long long)lay.blocks.size());
    for (auto &b : lay.blocks) { mix(b.first); mix(b.second); }
    lay.fp = v;
    return lay;
}

QpCache qp_cache(pbd_qp *q)
{
    QpCache c{};
    c.x = q->x.as<float>(); c.bm = q->bm.as<uint8_t>(); c.hd = q->hd.as<int32_t>(); c.ids = q->ids.as<int32_t>();
    c.b = q->b.as<double>(); c.d = q->d.as<double>(); c.a = q->a.as<double>(); c.sv = q->sv.as<uint8_t>();
    c.cap = q->cap; c.V = q->V; c.HW = q->HW; c.MB = q->MB;
    c.w = q->w.as<double>(); c.wreg = q->wreg.p; c.w0 = q->w0.p;
    c.noneg = q->noneg.p; c.nnoneg = q->nnoneg; c.L = q->L;
    c.slot_of = q->slot_of.p; c.slot_len = q->slot_len.p;
    return c;
}

// a header of pbd_examples' format: -1 marked invalid, 0 not a valid example for this layout, 1 valid
int qp_header_ok(const pbd_qp *q, const int32_t *h)
{
    const int nb = h[2], nv = h[3];
    if (nb == -1) return -1;
    if (nb < 0 || nb > (q->in_hw - 4) / 2 || nb > q->MB || nv < 0 || nv > q->V) return 0;
    long long tot = 0;
    for (int b = 0; b < nb; ++b) {
        const int off = h[4 + 2 * b], len = h[5 + 2 * b];
        if (off < 0 || off >= q->L) return 0;
        const int s = q->slot_of_h[off];
        if (s < 0 || q->slot_len_h[s] != len) return 0;
        tot += len;
    }
    return tot == nv ? 1 : 0;
}

// the write of m examples already on the device (p's inputs set), then the host mirror of the new entries
int qp_write(pbd_qp *q, QpWriteParams &p, bool f64, int *taken)
{
    p.c = qp_cache(q);
    p.in_hw = q->in_hw; p.in_vs = q->V; p.n0 = q->n; p.Cpos = q->Cpos; p.Cneg = q->Cneg;
    QPCHK(q, q->work.ensure((size_t)std::max(p.m, 1) * sizeof(int)));
    p.slot = q->work.as<int>();
    p.taken = q->misc.as<int>();
    launch_qp_write(p, f64, q->stream);
    QPCHK(q, hipGetLastError());
    int t = 0;
    QPCHK(q, hipMemcpyAsync(&t, p.taken, sizeof(int), hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    if (t < 0 || t > q->cap - q->n) return qp_fail(q, PBD_ERR_HIP, "the write reported %d entries", t);
    const int n0 = q->n, n1 = q->n + t;
    q->h_ids.resize((size_t)n1 * 5);
    q->h_hd.resize((size_t)n1 * q->HW);
    q->h_b.resize(n1);
    if (t > 0) {
        QPCHK(q, hipMemcpyAsync(&q->h_ids[(size_t)n0 * 5], q->ids.as<int32_t>() + (size_t)n0 * 5, (size_t)t * 5 * sizeof(int32_t),
                                hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipMemcpyAsync(&q->h_hd[(size_t)n0 * q->HW], q->hd.as<int32_t>() + (size_t)n0 * q->HW,
                                (size_t)t * q->HW * sizeof(int32_t), hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipMemcpyAsync(&q->h_b[n0], q->b.as<double>() + n0, (size_t)t * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
    }
    q->n = n1;
    if (taken) *taken = t;
    return PBD_OK;
}

// group numbers of the entries list[0..k) (ascending indices): equal ids share a group, groups numbered by first member
std::vector<int> qp_groups(const pbd_qp *q, const std::vector<int> &list, int *ngroups)
{
    std::map<std::array<int32_t, 5>, int> seen;
    std::vector<int> g(list.size());
    for (size_t k = 0; k < list.size(); ++k) {
        std::array<int32_t, 5> id;
        for (int c = 0; c < 5; ++c) id[c] = q->h_ids[(size_t)list[k] * 5 + c];
        auto it = seen.emplace(id, (int)seen.size()).first;
        g[k] = it->second;
    }
    *ngroups = (int)seen.size();
    return g;
}

// qp_refresh: w and l from a (lincomb's order), the clamps, lb
int qp_refresh(pbd_qp *q)
{
    // every QP call works on q->stream (created non-blocking, or the caller's): the duals are read in its order, after all
    // work queued before (prune's compaction in particular)
    std::vector<double> a(q->n);
    if (q->n) QPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    std::vector<int> P;
    for (int i = 0; i < q->n; ++i) if (a[i] > 0) P.push_back(i);
    std::stable_sort(P.begin(), P.end(), [&](int u, int v) { return a[u] < a[v]; });
    double l = 0.0;
    for (int i : P) l = l + q->h_b[i] * a[i];
    // the entries carrying each layout block, in P's order
    const int nslots = (int)q->slot_len_h.size();
    std::vector<std::vector<int2> > per(nslots);
    for (int i : P) {
        const int32_t *h = &q->h_hd[(size_t)i * q->HW];
        for (int b = 0; b < h[0]; ++b) per[q->slot_of_h[h[2 + 3 * b]]].push_back(make_int2(i, h[4 + 3 * b]));
    }
    std::vector<QpTask> tasks;
    std::vector<int2> ent;
    for (int s = 0; s < nslots; ++s) {
        if (per[s].empty()) continue;
        const int begin = (int)ent.size();
        ent.insert(ent.end(), per[s].begin(), per[s].end());
        const int off = q->slot_off_h[s];
        for (int c0 = 0; c0 < q->slot_len_h[s]; c0 += PBD_QP_LANES)
            tasks.push_back(QpTask{off, c0, std::min(PBD_QP_LANES, q->slot_len_h[s] - c0), begin, (int)ent.size(), 0});
    }
    const size_t tb = (tasks.size() * sizeof(QpTask) + 255) / 256 * 256;
    QPCHK(q, q->lc.ensure(tb + ent.size() * sizeof(int2) + 16));
    if (!tasks.empty()) {
        QPCHK(q, hipMemcpyAsync(q->lc.p, tasks.data(), tasks.size() * sizeof(QpTask), hipMemcpyHostToDevice, q->stream));
        QPCHK(q, hipMemcpyAsync(q->lc.as<char>() + tb, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, q->stream));
    }
    QpLincombParams lp{};
    lp.c = qp_cache(q);
    lp.tasks = q->lc.as<QpTask>(); lp.ntasks = (int)tasks.size();
    lp.ent = reinterpret_cast<const int2 *>(q->lc.as<char>() + tb);
    lp.ww = q->misc.as<double>() + 1;
    launch_qp_lincomb(lp, q->stream);
    QPCHK(q, hipGetLastError());
    double ww = 0;
    QPCHK(q, hipMemcpyAsync(&ww, lp.ww, sizeof(double), hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    const double lb = l - ww * 0.5;
    if (q->have_lb && !(lb > q->lb - 1e-5)) q->lb_dropped = 1;
    q->l = l; q->ww = ww; q->lb = lb; q->have_lb = true;
    return PBD_OK;
}

// G = R(w . x) - b of every entry, then computeloss over the whole cache
int qp_true_loss(pbd_qp *q, double *loss)
{
    QPCHK(q, q->work.ensure((size_t)std::max(q->n, 1) * sizeof(double)));
    QpScoreParams sp{};
    sp.c = qp_cache(q); sp.w = q->w.as<double>(); sp.first = 0; sp.count = q->n; sp.sub_b = 1; sp.scale = 1.0;
    sp.out = q->work.as<double>();
    launch_qp_score(sp, q->stream);
    QPCHK(q, hipGetLastError());
    std::vector<double> G(q->n);
    if (q->n) QPCHK(q, hipMemcpyAsync(G.data(), sp.out, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    std::vector<int> all(q->n);
    std::iota(all.begin(), all.end(), 0);
    int ng = 0;
    const std::vector<int> g = qp_groups(q, all, &ng);
    std::vector<double> best(ng, 0.0);   // max(0, max slack) of every group
    for (int i = 0; i < q->n; ++i) {
        const double slack = -G[i];
        if (slack > best[g[i]]) best[g[i]] = slack;
    }
    double s = 0.0;
    for (int k = 0; k < ng; ++k) if (best[k] > 0) s = s + best[k];
    *loss = s;
    return PBD_OK;
}

uint64_t qp_splitmix64(uint64_t seed, uint64_t i)
{
    const uint64_t base = seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL;
    uint64_t z = base + i * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int qp_set_sv(pbd_qp *q, int count)
{
    if (count > 0) QPCHK(q, hipMemsetAsync(q->sv.p, 1, (size_t)count, q->stream));
    return PBD_OK;
}

// qp_one: the pass over the support vectors, refresh, the fixed set's sv, lb and ub
int qp_one(pbd_qp *q, const int32_t *order, int norder, uint64_t seed)
{
    std::vector<double> a(q->n);
    std::vector<uint8_t> sv(q->n);
    if (q->n) {
        QPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
    }
    std::vector<int> S;
    for (int i = 0; i < q->n; ++i) if (sv[i]) S.push_back(i);
    const int nsv = (int)S.size();
    if (nsv == 0) return qp_fail(q, PBD_ERR_STATE, "no support vectors (empty cache)");
    std::vector<int> perm(nsv);
    if (order) {
        if (norder != nsv) return qp_fail(q, PBD_ERR_INVALID, "order of %d indices, %d support vectors", norder, nsv);
        std::vector<char> used(nsv, 0);
        for (int k = 0; k < nsv; ++k) {
            if (order[k] < 0 || order[k] >= nsv || used[order[k]]) return qp_fail(q, PBD_ERR_INVALID, "order is not a permutation of 0..%d", nsv - 1);
            used[order[k]] = 1;
            perm[k] = order[k];
        }
    } else {
        std::vector<uint64_t> z(nsv);
        for (int k = 0; k < nsv; ++k) z[k] = qp_splitmix64(seed, (uint64_t)k + 1);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int u, int v) { return z[u] < z[v]; });
    }
    int ng = 0;
    const std::vector<int> gS = qp_groups(q, S, &ng);
    std::vector<double> idC(ng, 0.0);
    std::vector<int> idI(ng, -1);
    for (int k = 0; k < nsv; ++k) {
        idC[gS[k]] = idC[gS[k]] + a[S[k]];
        if (a[S[k]] > 0) idI[gS[k]] = S[k];
    }
    std::vector<int> ord(nsv), gidx(nsv);
    for (int k = 0; k < nsv; ++k) { ord[k] = S[perm[k]]; gidx[k] = gS[perm[k]]; }
    // work: order, gidx (int), idC, err (double), idI (int)
    const size_t o_ord = 0, o_g = o_ord + (size_t)nsv * 4, o_c = (o_g + (size_t)nsv * 4 + 7) / 8 * 8, o_e = o_c + (size_t)ng * 8,
                 o_i = o_e + (size_t)ng * 8, tot = o_i + (size_t)ng * 4;
    QPCHK(q, q->work.ensure(tot + 16));
    char *wb = q->work.as<char>();
    QPCHK(q, hipMemcpyAsync(wb + o_ord, ord.data(), (size_t)nsv * 4, hipMemcpyHostToDevice, q->stream));
    QPCHK(q, hipMemcpyAsync(wb + o_g, gidx.data(), (size_t)nsv * 4, hipMemcpyHostToDevice, q->stream));
    QPCHK(q, hipMemcpyAsync(wb + o_c, idC.data(), (size_t)ng * 8, hipMemcpyHostToDevice, q->stream));
    QPCHK(q, hipMemsetAsync(wb + o_e, 0, (size_t)ng * 8, q->stream));
    QPCHK(q, hipMemcpyAsync(wb + o_i, idI.data(), (size_t)ng * 4, hipMemcpyHostToDevice, q->stream));
    QpPassParams pp{};
    pp.c = qp_cache(q);
    pp.order = reinterpret_cast<const int *>(wb + o_ord); pp.gidx = reinterpret_cast<const int *>(wb + o_g);
    pp.nsteps = nsv; pp.ngroups = ng;
    pp.idC = reinterpret_cast<double *>(wb + o_c); pp.err = reinterpret_cast<double *>(wb + o_e);
    pp.idI = reinterpret_cast<int *>(wb + o_i);
    pp.loss = q->misc.as<double>() + 2;
    launch_qp_pass(pp, q->stream);
    QPCHK(q, hipGetLastError());
    double loss = 0;
    QPCHK(q, hipMemcpyAsync(&loss, pp.loss, sizeof(double), hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    if (int rc = qp_refresh(q)) return rc;
    if (int rc = qp_set_sv(q, q->nfix)) return rc;
    q->loss = loss;
    q->ub = q->ww * 0.5 + loss;
    return PBD_OK;
}

void qp_fill_state(const pbd_qp *q, pbd_qp_info *st, int nsv)
{
    if (!st) return;
    *st = pbd_qp_info{};
    st->n = q->n; st->nsv = nsv; st->nfix = q->nfix; st->capacity = q->cap; st->len = q->L; st->hdr_words = q->HW; st->values = q->V;
    st->lb = q->lb; st->ub = q->ub; st->loss = q->loss; st->l = q->l;
    st->lb_dropped = q->lb_dropped; st->passes = q->passes; st->converged = q->converged;
}

int qp_count_sv(pbd_qp *q, int *nsv)
{
    std::vector<uint8_t> sv(q->n);
    if (q->n) QPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
    QPCHK(q, hipStreamSynchronize(q->stream));
    int k = 0;
    for (uint8_t v : sv) k += v ? 1 : 0;
    *nsv = k;
    return PBD_OK;
}

}  // namespace

extern "C" {

int pbd_qp_create(const pbd_handle *h, const struct pbd_qp_config *cfg, pbd_qp **out)
{
    try {
        if (!h || !cfg || !out) return qp_fail(nullptr, PBD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (cfg->capacity <= 0) return qp_fail(nullptr, PBD_ERR_INVALID, "capacity %d (at least 1)", cfg->capacity);
        const double C = cfg->C == 0 ? 0.002 : cfg->C, wpos = cfg->wpos == 0 ? 2.0 : cfg->wpos;
        if (!(C > 0) || !std::isfinite(C) || !(wpos > 0) || !std::isfinite(wpos))
            return qp_fail(nullptr, PBD_ERR_INVALID, "C %g and wpos %g must be finite and positive", cfg->C, cfg->wpos);
        (void)hipSetDevice(h->cfg.device);
        std::unique_ptr<pbd_qp> q(new pbd_qp);
        q->device = h->cfg.device;
        const QpLayout lay = qp_layout(h);
        q->L = lay.L; q->V = lay.V; q->in_hw = lay.in_hw; q->fp = lay.fp;
        q->MB = (lay.in_hw - 4) / 2;
        if (q->MB > 256 || q->MB < 1) return qp_fail(nullptr, PBD_ERR_UNSUPPORTED, "examples of %d blocks (at most 256)", q->MB);
        if (q->V % 4) return qp_fail(nullptr, PBD_ERR_INVALID, "example stride %d", q->V);
        q->HW = 2 + 3 * q->MB;
        q->cap = cfg->capacity;
        q->Cpos = C * wpos; q->Cneg = C;
        q->slot_of_h.assign(q->L, -1);
        for (auto &b : lay.blocks) {
            if (b.first < 0 || b.first + (long long)b.second > q->L)
                return qp_fail(nullptr, PBD_ERR_INVALID, "layout block at %d of %d values outside w", b.first, b.second);
            if (q->slot_of_h[b.first] < 0) {
                q->slot_of_h[b.first] = (int)q->slot_len_h.size();
                q->slot_len_h.push_back(b.second);
                q->slot_off_h.push_back(b.first);
            }
        }
        // model2vec's defaults in this vector order
        q->wreg_h.assign(q->L, 1.0);
        q->w0_h.assign(q->L, 0.0);
        std::vector<int> nn;
        if (cfg->wreg) q->wreg_h.assign(cfg->wreg, cfg->wreg + q->L);
        else for (int c = 0; c < h->NC; ++c) q->wreg_h[h->biasid[h->mix_offset[h->part_offset[c]]]] = 0.01;
        if (cfg->w0) q->w0_h.assign(cfg->w0, cfg->w0 + q->L);
        else for (int d = 0; d < h->ndefs; ++d) { q->w0_h[h->nbias + 4 * d] = 0.01; q->w0_h[h->nbias + 4 * d + 2] = 0.01; }
        if (cfg->noneg) {
            if (cfg->nnoneg < 0) return qp_fail(nullptr, PBD_ERR_INVALID, "nnoneg %d", cfg->nnoneg);
            for (int k = 0; k < cfg->nnoneg; ++k) {
                if (cfg->noneg[k] < 0 || cfg->noneg[k] >= q->L) return qp_fail(nullptr, PBD_ERR_INVALID, "noneg index %d", cfg->noneg[k]);
                nn.push_back(cfg->noneg[k]);
            }
        } else {
            for (int d = 0; d < h->ndefs; ++d) { nn.push_back(h->nbias + 4 * d); nn.push_back(h->nbias + 4 * d + 2); }
        }
        for (int k = 0; k < q->L; ++k)
            if (!std::isfinite(q->wreg_h[k]) || q->wreg_h[k] == 0 || !std::isfinite(q->w0_h[k]))
                return qp_fail(nullptr, PBD_ERR_INVALID, "wreg / w0 at %d: %g / %g (finite, wreg nonzero)", k, q->wreg_h[k], q->w0_h[k]);
        q->nnoneg = (int)nn.size();
        if (cfg->stream) q->stream.borrow(reinterpret_cast<hipStream_t>(cfg->stream));
        else QPCHK(nullptr, q->stream.create());
        const size_t cap = (size_t)q->cap;
        QPCHK(nullptr, qp_alloc(q->x, cap * q->V * sizeof(float)));
        QPCHK(nullptr, qp_alloc(q->bm, cap * q->V));
        QPCHK(nullptr, qp_alloc(q->hd, cap * q->HW * sizeof(int32_t)));
        QPCHK(nullptr, qp_alloc(q->ids, cap * 5 * sizeof(int32_t)));
        QPCHK(nullptr, qp_alloc(q->b, cap * sizeof(double)));
        QPCHK(nullptr, qp_alloc(q->d, cap * sizeof(double)));
        QPCHK(nullptr, qp_alloc(q->a, cap * sizeof(double)));
        QPCHK(nullptr, qp_alloc(q->sv, cap));
        QPCHK(nullptr, qp_alloc(q->w, (size_t)q->L * sizeof(double)));
        QPCHK(nullptr, qp_alloc(q->wraw, (size_t)q->L * sizeof(double)));
        QPCHK(nullptr, qp_alloc(q->misc, 4 * sizeof(double)));
        QPCHK(nullptr, hipMemsetAsync(q->w.p, 0, (size_t)q->L * sizeof(double), q->stream));
        QPCHK(nullptr, hipMemsetAsync(q->a.p, 0, cap * sizeof(double), q->stream));
        QPCHK(nullptr, hipMemsetAsync(q->sv.p, 0, cap, q->stream));
        QPCHK(nullptr, q->wreg.upload(q->wreg_h));
        QPCHK(nullptr, q->w0.upload(q->w0_h));
        if (!nn.empty()) QPCHK(nullptr, q->noneg.upload(nn));
        QPCHK(nullptr, q->slot_of.upload(q->slot_of_h));
        QPCHK(nullptr, q->slot_len.upload(q->slot_len_h));   // DevTable uploads are blocking copies
        QPCHK(nullptr, hipStreamSynchronize(q->stream));
        *out = q.release();
        return PBD_OK;
    } catch (const std::bad_alloc &) {
        return qp_fail(nullptr, PBD_ERR_NOMEM, "out of host memory");
    } catch (...) {
        return qp_fail(nullptr, PBD_ERR_INVALID, "unexpected exception");
    }
}

void pbd_qp_destroy(pbd_qp *q)
{
    if (!q) return;
    (void)hipSetDevice(q->device);
    (void)hipStreamSynchronize(q->stream);
    delete q;
}

const char *pbd_qp_last_error(const pbd_qp *q) { return q ? q->err.c_str() : g_create_error.c_str(); }

int pbd_qp_add(pbd_qp *q, const pbd_handle *h, int n, const int32_t *hdr, const void *values, const int32_t *ids, int *taken)
{
    return qp_entry(q, h && (n <= 0 || (hdr && values && ids)), [&]() -> int {
        if (n < 0) return qp_fail(q, PBD_ERR_INVALID, "n %d", n);
        if (qp_layout(h).fp != q->fp) return qp_fail(q, PBD_ERR_INVALID, "the handle's model-vector layout differs from the QP's");
        for (int e = 0; e < n; ++e)
            if (qp_header_ok(q, hdr + (size_t)e * q->in_hw) == 0)
                return qp_fail(q, PBD_ERR_INVALID, "example %d: a block that is not a block of the model vector, or bad counts", e);
        if (taken) *taken = 0;
        if (n == 0) return PBD_OK;
        const size_t rs = h->rs;
        const size_t hb = (size_t)n * q->in_hw * 4, vb = (size_t)n * q->V * rs, ib = (size_t)n * 5 * 4;
        const size_t o_v = (hb + 255) / 256 * 256, o_i = o_v + (vb + 255) / 256 * 256;
        QPCHK(q, q->stage.ensure(o_i + ib));
        QPCHK(q, hipMemcpyAsync(q->stage.p, hdr, hb, hipMemcpyHostToDevice, q->stream));
        QPCHK(q, hipMemcpyAsync(q->stage.as<char>() + o_v, values, vb, hipMemcpyHostToDevice, q->stream));
        QPCHK(q, hipMemcpyAsync(q->stage.as<char>() + o_i, ids, ib, hipMemcpyHostToDevice, q->stream));
        QpWriteParams p{};
        p.in_hdr = q->stage.as<int32_t>();
        p.in_values = q->stage.as<char>() + o_v;
        p.in_ids = reinterpret_cast<const int32_t *>(q->stage.as<char>() + o_i);
        p.m = n;
        return qp_write(q, p, h->f64, taken);
    });
}

int pbd_qp_add_device(pbd_qp *q, pbd_handle *h, const int32_t *d_payload, int capacity, const int32_t *d_hdr, const void *d_values,
                      int label, int id_base, int32_t *d_taken)
{
    return qp_entry(q, h && d_payload && (capacity <= 0 || (d_hdr && d_values)), [&]() -> int {
        if (capacity < 0) return qp_fail(q, PBD_ERR_INVALID, "capacity %d", capacity);
        if (qp_layout(h).fp != q->fp) return qp_fail(q, PBD_ERR_INVALID, "the handle's model-vector layout differs from the QP's");
        (void)hipSetDevice(q->device);
        if (h->stream.s != q->stream.s) {   // the QP's stream waits for the handle's
            Event ev;
            QPCHK(q, hipEventCreateWithFlags(&ev.p, hipEventDisableTiming));
            QPCHK(q, hipEventRecord(ev.p, h->stream));
            QPCHK(q, hipStreamWaitEvent(q->stream, ev.p, 0));
        }
        QpWriteParams p{};
        p.in_hdr = d_hdr; p.in_values = d_values; p.in_ids = nullptr;
        p.payload = d_payload; p.rec_stride = ::stride(h); p.label = label; p.id_base = id_base;
        p.m = capacity;
        p.taken_user = d_taken;
        if (capacity == 0) {
            if (d_taken) QPCHK(q, hipMemsetAsync(d_taken, 0, sizeof(int32_t), q->stream));
            QPCHK(q, hipStreamSynchronize(q->stream));
            return PBD_OK;
        }
        return qp_write(q, p, h->f64, nullptr);
    });
}

int pbd_qp_fix(pbd_qp *q)
{
    return qp_entry(q, true, [&]() -> int {
        q->nfix = q->n;
        if (int rc = qp_set_sv(q, q->n)) return rc;
        QPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

int pbd_qp_prune(pbd_qp *q, int *n)
{
    return qp_entry(q, true, [&]() -> int {
        q->lb_dropped = 0;
        std::vector<double> a(q->n);
        std::vector<uint8_t> sv(q->n);
        if (q->n) {
            QPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
            QPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
            QPCHK(q, hipStreamSynchronize(q->stream));
        }
        bool all = true;
        for (uint8_t v : sv) all = all && v;
        if (all) for (int i = 0; i < q->n; ++i) sv[i] = (a[i] > 0 || i < q->nfix) ? 1 : 0;
        std::vector<int> I;
        for (int i = 0; i < q->n; ++i) if (sv[i]) I.push_back(i);
        const int n1 = (int)I.size();
        if (n1 == 0) return qp_fail(q, PBD_ERR_STATE, "nothing to keep (empty cache)");
        int first = 0;
        while (first < n1 && I[first] == first) ++first;
        // compaction in ascending chunks of at most `chunk` entries through a scratch buffer freed afterwards: a chunk's sources
        // I[k] >= k lie at or past the chunk's own start and past every earlier chunk's destinations, so each chunk reads
        // entries no earlier chunk has overwritten
        const size_t V = q->V, HW = q->HW;
        const size_t entry_bytes = V * 5 + HW * 4 + 20 + 3 * 8;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)std::max(n1 - first, 1), kQpPruneChunkEntries),
                                                                     kQpPruneChunkBytes / entry_bytes));
        if (first < n1) {
            const size_t c = (size_t)chunk;
            const size_t o_x = 0, o_bm = o_x + c * V * 4, o_hd = (o_bm + c * V + 255) / 256 * 256, o_id = o_hd + c * HW * 4,
                         o_b = (o_id + c * 20 + 255) / 256 * 256, o_d = o_b + c * 8, o_a = o_d + c * 8, tot = o_a + c * 8;
            QPCHK(q, qp_alloc(q->scratch, tot));
            QPCHK(q, q->work.ensure((size_t)(n1 - first) * sizeof(int)));
            QPCHK(q, hipMemcpyAsync(q->work.p, &I[first], (size_t)(n1 - first) * sizeof(int), hipMemcpyHostToDevice, q->stream));
            char *s = q->scratch.as<char>();
            for (int k0 = first; k0 < n1; k0 += chunk) {
                const size_t cnt = (size_t)std::min(chunk, n1 - k0), k = (size_t)k0;
                QpGatherParams gp{};
                gp.c = qp_cache(q); gp.src = q->work.as<int>() + (k0 - first); gp.count = (int)cnt; gp.dst0 = k0;
                gp.x = reinterpret_cast<float *>(s + o_x); gp.bm = reinterpret_cast<uint8_t *>(s + o_bm);
                gp.hd = reinterpret_cast<int32_t *>(s + o_hd); gp.ids = reinterpret_cast<int32_t *>(s + o_id);
                gp.b = reinterpret_cast<double *>(s + o_b); gp.d = reinterpret_cast<double *>(s + o_d);
                gp.a = reinterpret_cast<double *>(s + o_a);
                launch_qp_gather(gp, q->stream);
                QPCHK(q, hipGetLastError());
                auto back = [&](void *dst, size_t off, size_t bytes) {
                    return hipMemcpyAsync(dst, s + off, bytes, hipMemcpyDeviceToDevice, q->stream);
                };
                QPCHK(q, back(q->x.as<float>() + k * V, o_x, cnt * V * 4));
                QPCHK(q, back(q->bm.as<uint8_t>() + k * V, o_bm, cnt * V));
                QPCHK(q, back(q->hd.as<int32_t>() + k * HW, o_hd, cnt * HW * 4));
                QPCHK(q, back(q->ids.as<int32_t>() + k * 5, o_id, cnt * 20));
                QPCHK(q, back(q->b.as<double>() + k, o_b, cnt * 8));
                QPCHK(q, back(q->d.as<double>() + k, o_d, cnt * 8));
                QPCHK(q, back(q->a.as<double>() + k, o_a, cnt * 8));
            }
            QPCHK(q, hipStreamSynchronize(q->stream));
            q->scratch = DevBuf{};
        }
        int nfix = 0;
        for (int k = 0; k < n1; ++k) {
            const int i = I[k];
            if (i < q->nfix) ++nfix;
            if (k != i) {
                std::copy_n(&q->h_ids[(size_t)i * 5], 5, &q->h_ids[(size_t)k * 5]);
                std::copy_n(&q->h_hd[(size_t)i * q->HW], q->HW, &q->h_hd[(size_t)k * q->HW]);
                q->h_b[k] = q->h_b[i];
            }
        }
        q->h_ids.resize((size_t)n1 * 5); q->h_hd.resize((size_t)n1 * q->HW); q->h_b.resize(n1);
        q->n = n1; q->nfix = nfix;
        if (q->cap > n1) QPCHK(q, hipMemsetAsync(q->sv.as<uint8_t>() + n1, 0, (size_t)(q->cap - n1), q->stream));
        if (int rc = qp_set_sv(q, n1)) return rc;
        if (int rc = qp_refresh(q)) return rc;
        if (n) *n = n1;
        return PBD_OK;
    });
}

int pbd_qp_one(pbd_qp *q, const int32_t *order, int norder, uint64_t seed, struct pbd_qp_info *state)
{
    return qp_entry(q, true, [&]() -> int {
        q->lb_dropped = 0;
        if (int rc = qp_one(q, order, norder, seed)) return rc;
        q->passes = 1; q->converged = 0;
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_opt(pbd_qp *q, double tol, int iter, uint64_t seed, struct pbd_qp_info *state)
{
    return qp_entry(q, true, [&]() -> int {
        if (std::isnan(tol)) return qp_fail(q, PBD_ERR_INVALID, "tol is NaN");
        if (iter < 0) return qp_fail(q, PBD_ERR_INVALID, "iter %d", iter);
        if (q->n == 0) return qp_fail(q, PBD_ERR_STATE, "empty cache");
        q->lb_dropped = 0; q->passes = 0; q->converged = 0;
        if (int rc = qp_refresh(q)) return rc;
        double loss = 0;
        if (int rc = qp_true_loss(q, &loss)) return rc;
        double ub = q->ww * 0.5 + loss;
        if (int rc = qp_set_sv(q, q->n)) return rc;
        for (int t = 0; t < iter; ++t) {
            if (int rc = qp_one(q, nullptr, 0, seed + (uint64_t)t)) return rc;
            q->passes = t + 1;
            const double lb = q->lb, ub_est = ub < q->ub ? ub : q->ub;
            if (lb > 0 && 1 - lb / ub_est < tol) {
                if (int rc = qp_true_loss(q, &loss)) return rc;
                const double u = q->ww * 0.5 + loss;
                ub = u < ub ? u : ub;
                if (1 - lb / ub < tol) { q->converged = 1; break; }
                if (int rc = qp_set_sv(q, q->n)) return rc;
            }
        }
        q->ub = ub;
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_weights(pbd_qp *q, double *w)
{
    return qp_entry(q, w != nullptr, [&]() -> int {
        std::vector<double> v(q->L);
        QPCHK(q, hipMemcpyAsync(v.data(), q->w.p, (size_t)q->L * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
        for (int k = 0; k < q->L; ++k) w[k] = v[k] / q->wreg_h[k] + q->w0_h[k];
        return PBD_OK;
    });
}

int pbd_qp_scores(pbd_qp *q, double *s, int *n)
{
    return qp_entry(q, s && n, [&]() -> int {
        std::vector<int> pos;
        for (int i = 0; i < q->n; ++i) if (q->h_ids[(size_t)i * 5] > 0) pos.push_back(i);
        *n = (int)pos.size();
        if (pos.empty()) return PBD_OK;
        const size_t o_o = ((size_t)pos.size() * 4 + 255) / 256 * 256;
        QPCHK(q, q->work.ensure(o_o + pos.size() * 8));
        QPCHK(q, hipMemcpyAsync(q->work.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, q->stream));
        QpCache c = qp_cache(q);
        launch_qp_wraw(c, q->wraw.as<double>(), q->stream);
        QpScoreParams sp{};
        sp.c = c; sp.w = q->wraw.as<double>(); sp.list = q->work.as<int>(); sp.count = (int)pos.size(); sp.sub_b = 0; sp.scale = q->Cpos;
        sp.out = reinterpret_cast<double *>(q->work.as<char>() + o_o);
        launch_qp_score(sp, q->stream);
        QPCHK(q, hipGetLastError());
        QPCHK(q, hipMemcpyAsync(s, sp.out, pos.size() * 8, hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

int pbd_qp_state(pbd_qp *q, struct pbd_qp_info *state, double *a, uint8_t *sv, double *w)
{
    return qp_entry(q, true, [&]() -> int {
        if (a && q->n) QPCHK(q, hipMemcpyAsync(a, q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        if (sv && q->n) QPCHK(q, hipMemcpyAsync(sv, q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
        if (w) QPCHK(q, hipMemcpyAsync(w, q->w.p, (size_t)q->L * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_entries(pbd_qp *q, int first, int count, int32_t *hdr, float *values, double *b, double *d, int32_t *ids)
{
    return qp_entry(q, true, [&]() -> int {
        if (first < 0 || count < 0 || (long long)first + count > q->n)
            return qp_fail(q, PBD_ERR_INVALID, "entries %d..%d of %d", first, first + count - 1, q->n);
        const size_t f = first, c = count;
        if (c == 0) return PBD_OK;
        if (hdr) QPCHK(q, hipMemcpyAsync(hdr, q->hd.as<int32_t>() + f * q->HW, c * q->HW * 4, hipMemcpyDeviceToHost, q->stream));
        if (values) QPCHK(q, hipMemcpyAsync(values, q->x.as<float>() + f * q->V, c * q->V * 4, hipMemcpyDeviceToHost, q->stream));
        if (b) QPCHK(q, hipMemcpyAsync(b, q->b.as<double>() + f, c * 8, hipMemcpyDeviceToHost, q->stream));
        if (d) QPCHK(q, hipMemcpyAsync(d, q->d.as<double>() + f, c * 8, hipMemcpyDeviceToHost, q->stream));
        if (ids) QPCHK(q, hipMemcpyAsync(ids, q->ids.as<int32_t>() + f * 5, c * 20, hipMemcpyDeviceToHost, q->stream));
        QPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

}  // extern "C"
