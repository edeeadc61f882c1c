// pbd_kernels_depthprune.hip -- opt-in scale-depth plausibility of root boxes (pbd_set_depth_prune, pbd_depth_prune*): the
// intent of SearchSpacePruning<T>::filterResponseByDepth (src/SearchSpacePruning.cpp:47-70), the stub detect(im, depth) leaves
// commented out (src/PartsBasedDetector.cpp:86-93): a root box w pixels wide of an object `width` wide must stand at depth
// Z = fx * width / w.  The rule is the project's and is stated once in include/pbd.h; depth_plausible below is its one device
// statement, and both kernels call it.
//
//   k_depth_prune_roots<R, D>   one thread per root cell of rootv ([frame][level][component][y][x]): a cell that is not above the
//                               threshold writes 0 and reads nothing else (most cells); the others build the root's rectangle as
//                               the walk does (part_rect<R>, pbd_dp.h) and write 1 or 0.  The find then also asks for the byte
//   k_depth_prune_records<D>    one thread per record of a payload: the rule on the record's own root rectangle, a flag per
//                               record and the kept count per 256; the depth-consistency filter's ordered compaction
//                               (launch_dc_emit) then writes the kept records
// Nine loads and comparisons per tested box: no LDS, no scratch, nothing depends on the box size.  Neither grid is capped.
#include "pbd_device.h"
#include "pbd_dp.h"

#include <algorithm>

namespace pbd {
namespace {

constexpr int kDprThreads = 256;      // = the compaction's records per block (dc_record_blocks)
constexpr int kDprWaves = kDprThreads / 64;

// sample (py, px) of a depth image of code D, widened to double (exact for every code)
template <int D> __device__ inline double depth_at(const Box3dFrame &fr, long long py, long long px)
{
    const uint8_t *row = fr.data + (size_t)py * (size_t)fr.pitch;
    if (D == kDepth8U) return (double)row[px];
    if (D == kDepth16U) return (double)reinterpret_cast<const uint16_t *>(row)[px];
    if (D == kDepth32F) return (double)reinterpret_cast<const float *>(row)[px];
    return reinterpret_cast<const double *>(row)[px];
}

// plausible(rect, depth, fx, width, tol) of include/pbd.h, step for step; 64-bit integers, so that x + w cannot wrap
template <int D>
__device__ inline bool depth_plausible(long long x, long long y, long long w, long long h, const Box3dFrame &fr, const DepthPruneRule &r)
{
    if (w <= 0) return true;
    const long long x1 = max(x, 0LL), y1 = max(y, 0LL);
    const long long x2 = min(x + w, (long long)fr.cols), y2 = min(y + h, (long long)fr.rows);
    if (x2 - x1 <= 0 || y2 - y1 <= 0) return true;
    const double Z = __ddiv_rn(__dmul_rn(r.fx, r.width), (double)w), band = __dmul_rn(r.tol, Z);
    bool valid = false, in_band = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const long long py = y1 + ((2 * j + 1) * (y2 - y1)) / 6;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const long long px = x1 + ((2 * i + 1) * (x2 - x1)) / 6;
            const double d = depth_at<D>(fr, py, px);
            const bool v = d > 0 && d < (double)INFINITY;          // NaN, zeros, negatives and Inf are holes
            valid = valid || v;
            in_band = in_band || (v && fabs(__dsub_rn(d, Z)) <= band);
        }
    }
    return !valid || in_band;         // unknown depth never prunes
}

template <typename R, int D>
__global__ __launch_bounds__(kDprThreads) void k_depth_prune_roots(ArgminParams p, DepthPruneRoots a)
{
    const long long o = (long long)blockIdx.x * kDprThreads + threadIdx.x;
    if (o >= p.ntotal) return;
    bool ok = false;
    if (static_cast<const R *>(p.rootv)[o] > (R)p.thresh) {          // the find's own expression (NaN compares false)
        const long long per_frame = p.cell_per_frame * p.NC;
        const int frame = (int)(o / per_frame);
        const RootCell rc = root_cell(p.lv, 0, p.nlevels, p.NC, o - (long long)frame * per_frame);
        const int ks = p.walk[p.walk_off[rc.comp]].ksize[p.rooti[o]];
        const PartRect r = part_rect<R>(rc.x, rc.y, ks, (R)p.scales[rc.level], p.lv[rc.level]);
        const int w = r.x2 - r.x1, h = r.y2 - r.y1;                  // the words k_argmin_walk writes
        ok = depth_plausible<D>(r.x1, r.y1, w, h, a.frames[p.lv_frame ? p.lv_frame[rc.level] : frame], a.rule);
    }
    a.ok[o] = ok ? 1 : 0;
}

template <int D>
__global__ __launch_bounds__(kDprThreads) void k_depth_prune_records(DcParams p, DepthPruneRule rule)
{
    __shared__ int partial[kDprWaves];
    const int i = blockIdx.x * kDprThreads + threadIdx.x;
    int keep = 0;
    if (i < dc_count(p)) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        const long long f = (long long)r[kRecFrame] - p.frame_offset;
        const int n = r[kRecNparts];
        if (f >= 0 && f < p.nframes && n >= 1 && n <= p.max_parts) {   // any other record is dropped
            const int32_t *q = record_part(r, 0);
            keep = depth_plausible<D>(q[0], q[1], q[2], q[3], p.frames[f], rule) ? 1 : 0;
        }
    }
    p.flag[i] = keep;   // [blocks * kDprThreads]
    const int tot = block_sum<kDprWaves, int>(keep, partial);
    if (threadIdx.x == 0) p.blk[blockIdx.x] = tot;
}

template <class F> void for_depth(int depth, F &&f)
{
    switch (depth) {
    case kDepth8U: f(std::integral_constant<int, kDepth8U>{}); break;
    case kDepth16U: f(std::integral_constant<int, kDepth16U>{}); break;
    case kDepth32F: f(std::integral_constant<int, kDepth32F>{}); break;
    default: f(std::integral_constant<int, kDepth64F>{}); break;
    }
}

}  // namespace

void launch_depth_prune_roots(const ArgminParams &p, const DepthPruneRoots &a, bool f64, hipStream_t s)
{
    if (p.ntotal <= 0) return;
    const dim3 grid((unsigned)((p.ntotal + kDprThreads - 1) / kDprThreads));
    for_depth(a.depth, [&](auto d) {
        if (f64) PBD_LAUNCH((k_depth_prune_roots<double, decltype(d)::value>), grid, dim3(kDprThreads), 0, s, p, a);
        else PBD_LAUNCH((k_depth_prune_roots<float, decltype(d)::value>), grid, dim3(kDprThreads), 0, s, p, a);
    });
}

void launch_depth_prune_records(const DcParams &p, const DepthPruneRule &rule, hipStream_t s)
{
    for_depth(p.depth, [&](auto d) {
        PBD_LAUNCH(k_depth_prune_records<decltype(d)::value>, dim3(dc_record_blocks(p.in_cap)), dim3(kDprThreads), 0, s, p, rule);
    });
    launch_dc_emit(p, s);
}

}  // namespace pbd
