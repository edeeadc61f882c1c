// pbd_kernels_gridnms.hip -- opt-in grid maxima of a set of planes (pbd_grid_nms*, pbd_set_root_nms):
// nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129), the block NMS of Neubeck and Van Gool the reference's
// detect() calls on rootv between min and argmin and leaves commented out (src/PartsBasedDetector.cpp:86).
//
//   k_grid_nms<R, Elig, W>   one group of W lanes per block of (sz + 1) x (sz + 1) cells, W = 64 (a wave) or 1 (a thread):
//       1. the group's lanes stride over the block's cells; a reduction over (value, raster index) -- largest value, then
//          smallest index -- gives the candidate.  The order is total, so the result does not depend on the lane a cell fell to
//       2. the lanes stride over the window of 2 sz + 1 cells around the candidate, the cells of the candidate's own block
//          left out; a vote says whether an eligible cell is >= the candidate, and ends the scan
//       3. the block's bytes of dst are written: 255 at a kept candidate, 0 elsewhere -- the blocks tile the plane, so dst needs no
//          clearing pass
//     Elig says which cells take part: every one that is not NaN, those with a non-zero mask byte, or those above a threshold
//     (the detect path: `rootv > thresh`, the find's own expression, so no mask plane is ever written; with pbd_set_depth_prune
//     those above the threshold whose byte of the plausibility plane is set).
// Nothing is staged in LDS and nothing depends on sz but the loops' lengths: any sz runs.  The grid is capped; the groups
// stride over the (frame, plane, block) triples.
#include "pbd_device.h"

#include <algorithm>
#include <limits.h>

namespace pbd {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnMaxGrid = 2048;

struct GnAll {
    template <typename R> __device__ bool operator()(R v, size_t) const { return v == v; }
};
struct GnMask {
    const uint8_t *mask;
    template <typename R> __device__ bool operator()(R v, size_t i) const { return v == v && mask[i] != 0; }
};
template <typename R> struct GnAbove {
    R thresh;
    __device__ bool operator()(R v, size_t) const { return v > thresh; }   // NaN compares false
};
template <typename R> struct GnAboveMask {   // pbd_set_depth_prune with root NMS: the plausible cells above the threshold
    R thresh;
    const uint8_t *mask;
    __device__ bool operator()(R v, size_t i) const { return v > thresh && mask[i] != 0; }
};

// the better of two block candidates: an eligible one over none, the larger value, then the earlier cell
template <typename R> __device__ inline void gn_pick(R ov, int oe, R &v, int &e)
{
    if (oe >= 0 && (e < 0 || ov > v || (ov == v && oe < e))) { v = ov; e = oe; }
}

// whether any lane of the group says so
template <int W> __device__ inline bool gn_any(bool x)
{
    if (W == 1) return x;
    return __ballot(x) != 0ull;
}

// the window's cells outside [y0, y1) x [x0, x1), visited by the group's lanes; I: the type that holds the window's cell count
template <typename I, typename R, int W, class Elig>
__device__ inline bool gn_beaten(const R *src, size_t off, int cols, int wy0, int wx0, int wh, int ww, int y0, int y1, int x0, int x1,
                                 R best, const Elig &elig, int lane)
{
    const I n = (I)wh * ww;
    for (I e0 = 0; e0 < n; e0 += W) {
        const I e = e0 + lane;
        bool beats = false;
        if (e < n) {
            const int y = wy0 + (int)(e / ww), x = wx0 + (int)(e % ww);
            if (y < y0 || y >= y1 || x < x0 || x >= x1) {
                const size_t i = off + (size_t)y * cols + x;
                const R v = src[i];
                beats = elig(v, i) && !(best > v);
            }
        }
        if (gn_any<W>(beats)) return true;
    }
    return false;
}

template <typename R, class Elig, int W>
__global__ __launch_bounds__(kGnThreads) void k_grid_nms(GridNmsParams p, Elig elig)
{
    const R *src = static_cast<const R *>(p.src);
    const int lane = W == 1 ? 0 : (int)(threadIdx.x & 63), bs = p.sz + 1;
    const long long ngroups = (long long)gridDim.x * (kGnThreads / W);
    const long long total = p.blocks_per_frame * p.nframes;
    for (long long g = ((long long)blockIdx.x * kGnThreads + threadIdx.x) / W; g < total; g += ngroups) {
        const long long frame = g / p.blocks_per_frame, b = g - frame * p.blocks_per_frame;
        int lo = 0, hi = p.nplanes;                      // the last plane whose first block is <= b (empty planes share their
        while (hi - lo > 1) {                            // successor's and are skipped)
            const int mid = (lo + hi) >> 1;
            if (p.planes[mid].blk0 <= b) lo = mid; else hi = mid;
        }
        const GnPlane pl = p.planes[lo];
        const long long local = b - pl.blk0;
        const int by = (int)(local / pl.nbx), bx = (int)(local - (long long)by * pl.nbx);
        const size_t off = (size_t)frame * (size_t)p.frame_stride + (size_t)pl.off;
        const int y0 = by * bs, x0 = bx * bs, y1 = min(pl.rows - y0, bs) + y0, x1 = min(pl.cols - x0, bs) + x0;
        const int bw = x1 - x0, ncell = (y1 - y0) * bw;  // at most 2^30: sz <= 32767
        // 1. the block's candidate
        R best = 0;
        int bi = -1;
        for (int e = lane; e < ncell; e += W) {
            const size_t i = off + (size_t)(y0 + e / bw) * pl.cols + (x0 + e % bw);
            const R v = src[i];
            if (elig(v, i) && (bi < 0 || v > best)) { best = v; bi = e; }
        }
        if (W > 1) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) gn_pick<R>(__shfl_xor(best, d, 64), __shfl_xor(bi, d, 64), best, bi);
        }
        // 2. the candidate against its neighbourhood
        bool keep = bi >= 0;
        if (keep && p.sz > 0) {
            const int cy = y0 + bi / bw, cx = x0 + bi % bw;
            const int wy0 = max(cy - p.sz, 0), wx0 = max(cx - p.sz, 0);
            const int wh = (int)min((long long)cy + p.sz + 1, (long long)pl.rows) - wy0;
            const int ww = (int)min((long long)cx + p.sz + 1, (long long)pl.cols) - wx0;
            if ((long long)wh * ww <= INT_MAX)
                keep = !gn_beaten<int, R, W>(src, off, pl.cols, wy0, wx0, wh, ww, y0, y1, x0, x1, best, elig, lane);
            else
                keep = !gn_beaten<long long, R, W>(src, off, pl.cols, wy0, wx0, wh, ww, y0, y1, x0, x1, best, elig, lane);
        }
        // 3. the block's bytes
        for (int e = lane; e < ncell; e += W)
            p.dst[off + (size_t)(y0 + e / bw) * pl.cols + (x0 + e % bw)] = (keep && e == bi) ? (uint8_t)255 : (uint8_t)0;
    }
}

template <typename R, class Elig> void gn_launch(const GridNmsParams &p, const Elig &elig, int lanes, hipStream_t s)
{
    const long long total = p.blocks_per_frame * p.nframes;
    if (lanes == 1) {
        const int grid = (int)std::max<long long>(std::min<long long>((total + kGnThreads - 1) / kGnThreads, kGnMaxGrid), 1);
        PBD_LAUNCH((k_grid_nms<R, Elig, 1>), dim3(grid), dim3(kGnThreads), 0, s, p, elig);
    } else {
        const int per = kGnThreads / 64;
        const int grid = (int)std::max<long long>(std::min<long long>((total + per - 1) / per, kGnMaxGrid), 1);
        PBD_LAUNCH((k_grid_nms<R, Elig, 64>), dim3(grid), dim3(kGnThreads), 0, s, p, elig);
    }
}

}  // namespace

int grid_nms_lanes(int sz, int forced) { return forced ? forced : sz < kGnWaveSz ? 1 : 64; }

void launch_grid_nms(const GridNmsParams &p, bool f64, int lanes, hipStream_t s)
{
    if (p.blocks_per_frame <= 0 || p.nframes <= 0) return;
    auto run = [&](auto r) {
        using R = decltype(r);
        if (p.use_thresh && p.mask) gn_launch<R>(p, GnAboveMask<R>{(R)p.thresh, p.mask}, lanes, s);
        else if (p.use_thresh) gn_launch<R>(p, GnAbove<R>{(R)p.thresh}, lanes, s);
        else if (p.mask) gn_launch<R>(p, GnMask{p.mask}, lanes, s);
        else gn_launch<R>(p, GnAll{}, lanes, s);
    };
    if (f64) run(double{}); else run(float{});
}

}  // namespace pbd
