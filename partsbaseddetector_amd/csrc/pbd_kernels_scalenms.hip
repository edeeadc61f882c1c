// pbd_kernels_scalenms.hip -- opt-in suppression of a root's duplicates on neighbouring pyramid levels and components
// (pbd_set_scale_nms, pbd_scale_nms*): the scale-aware form of the call the reference's detect() leaves commented out,
// ssp_.nonMaxSuppression(rootv, scales) (src/PartsBasedDetector.cpp:86).  The rule is the project's and is stated once in
// include/pbd.h; sn_covers and sn_better below are its one device statement, and both kernels call them.
//
//   k_scale_nms<R>         a wave per span of 64 consecutive root cells of rootv ([frame][level][component][y][x]):
//       1. each lane reads its cell's score and mask bytes; a ballot gives the eligible cells of the span.  A span without one
//          (most spans at a real threshold) writes its 64 zero bytes and is done
//       2. the eligible lanes build their root's rectangle as the walk does (root_cell, rooti, part_rect<R>)
//       3. for each eligible root of the span in turn -- its cell, score and rectangle broadcast to the wave -- the 64 lanes
//          stride over the windows of the (2 dl + 1) * NC neighbouring planes.  A lane reads rootv and the mask bytes first and
//          builds a rectangle only for an eligible cell that is better than the root; the exact test then decides.  A wave vote
//          ends the root's scan at the first better neighbour
//       4. every lane writes its byte: 255 for eligible and kept, 0 otherwise -- every byte of dst is written
//     The window of a neighbour plane contains every neighbour (sn_window).  No LDS, no scratch.
//   k_scale_nms_records    one thread per record of a payload: the rule over the records of the record's frame (the list is
//                          grouped by ascending frame), a flag per record and the kept count per 256; the depth-consistency
//                          filter's ordered compaction (launch_dc_emit) then writes the kept records
#include "pbd_device.h"
#include "pbd_dp.h"

#include <algorithm>
#include <stddef.h>

namespace pbd {
namespace {

constexpr int kSnThreads = 256;       // = the compaction's records per block (dc_record_blocks)
constexpr int kSnWaves = kSnThreads / 64;
constexpr int kSnMaxGrid = 4096;
constexpr int kRecLevel = offsetof(pbd_candidate_hdr, level) / 4;

// covers(a, b) of include/pbd.h: b's centre, doubled, inside a's half-open rectangle; 64-bit, so that no caller's word can wrap
__device__ __forceinline__ bool sn_covers(long long xa, long long ya, long long wa, long long ha, long long xb, long long yb,
                                          long long wb, long long hb)
{
    const long long cx = 2 * xb + wb, cy = 2 * yb + hb;
    return wa > 0 && ha > 0 && 2 * xa <= cx && cx < 2 * (xa + wa) && 2 * ya <= cy && cy < 2 * (ya + ha);
}

// better(b, a): the larger score, then the earlier position in the find order (+0.0 and -0.0 tie; NaN is never asked)
template <typename S, typename I> __device__ __forceinline__ bool sn_better(S sb, I ib, S sa, I ia)
{
    return sb > sa || (sb == sa && ib < ia);
}

// The cells [c0, c1) of one axis of a neighbour plane (scale s, pad cells `pad`, n cells) that can hold a neighbour of a root whose
// rectangle spans [xa, xa + wa] on that axis, given that no rectangle of the plane is wider than wmax.
// A cell c of the plane has X = round((c - pad - 1) * s) and its rectangle starts at X or X - 1 and is wb <= wmax wide.
//   covers(a, b) needs 2 xa <= 2 xb + wb < 2 (xa + wa), so X >= xa - wmax / 2 and X - 1 < xa + wa
//   covers(b, a) needs 2 xb <= 2 xa + wa < 2 (xb + wb), so X - 1 <= xa + wa / 2 and X + wmax > xa + wa / 2
// Either way xa - wmax <= X <= xa + wa + 1.  X is monotone in c (s > 0), and round(t) in [lo, hi] puts t in [lo - 1/2, hi + 1/2];
// the product's rounding error in R is far below 1/2 for |X| < 2^31, so t in [lo - 1, hi + 1], and one more cell on either side
// absorbs the division's.  A scale that is not positive gives the whole axis.
__device__ __forceinline__ void sn_window(long long xa, long long wa, long long wmax, double s, int pad, int n, int &c0, int &c1)
{
    c0 = 0; c1 = n;
    if (!(s > 0)) return;
    const double lo = floor((double)(xa - wmax - 1) / s) + (double)pad, hi = ceil((double)(xa + wa + 2) / s) + (double)pad + 2.0;
    if (lo > 0) c0 = lo < (double)n ? (int)lo : n;
    if (hi < (double)(n - 1)) c1 = hi >= 0 ? (int)hi + 1 : 0;
}

template <typename R> __device__ __forceinline__ bool sn_eligible(const ScaleNmsRoots &a, const ArgminParams &p, long long o, R v)
{
    bool e = v > (R)p.thresh;                      // the find's own expression (NaN compares false)
    if (a.root_ok) e = e && a.root_ok[o] != 0;
    if (a.root_max) e = e && a.root_max[o] != 0;
    return e;
}

// the rectangle the walk writes for the root at (x, y) of level `level`, component `comp`, flat index o
template <typename R>
__device__ __forceinline__ void sn_root_rect(const ArgminParams &p, long long o, int level, int comp, int x, int y, int &rx, int &ry,
                                             int &rw, int &rh)
{
    const int ks = p.walk[p.walk_off[comp]].ksize[p.rooti[o]];
    const PartRect r = part_rect<R>(x, y, ks, (R)p.scales[level], p.lv[level]);
    rx = r.x1; ry = r.y1; rw = r.x2 - r.x1; rh = r.y2 - r.y1;
}

template <typename R>
__global__ __launch_bounds__(kSnThreads) void k_scale_nms(ArgminParams p, ScaleNmsRoots a)
{
    const R *rootv = static_cast<const R *>(p.rootv);
    const int lane = (int)(threadIdx.x & 63);
    const long long per_frame = p.cell_per_frame * p.NC;
    const long long nspans = (p.ntotal + 63) / 64, nwaves = (long long)gridDim.x * kSnWaves;
    for (long long span = (long long)blockIdx.x * kSnWaves + (threadIdx.x >> 6); span < nspans; span += nwaves) {
        // 1. the span's eligible cells
        const long long o = span * 64 + lane;
        R v = 0;
        bool elig = false;
        if (o < p.ntotal) { v = rootv[o]; elig = sn_eligible<R>(a, p, o, v); }
        unsigned long long todo = __ballot(elig);
        if (todo == 0ull) {
            if (o < p.ntotal) a.dst[o] = 0;
            continue;
        }
        // 2. their rectangles
        int frame = 0, level = 0, rx = 0, ry = 0, rw = 0, rh = 0;
        if (elig) {
            frame = (int)(o / per_frame);
            const RootCell rc = root_cell(p.lv, 0, p.nlevels, p.NC, o - (long long)frame * per_frame);
            level = rc.level;
            sn_root_rect<R>(p, o, rc.level, rc.comp, rc.x, rc.y, rx, ry, rw, rh);
        }
        // 3. each eligible root against its neighbourhood
        unsigned long long beaten_set = 0ull;
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const long long oa = span * 64 + j;
            const R sa = __shfl(v, j, 64);
            const int fa = __shfl(frame, j, 64), la = __shfl(level, j, 64);
            const int xa = __shfl(rx, j, 64), ya = __shfl(ry, j, 64), wa = __shfl(rw, j, 64), ha = __shfl(rh, j, 64);
            // the levels of a's frame within dl: its own pyramid, or the run of its frame's virtual levels
            int l0 = max(la - a.dl, 0), l1 = (int)min((long long)la + a.dl, (long long)p.nlevels - 1);
            if (p.lv_frame) {
                const int f = p.lv_frame[la];
                while (p.lv_frame[l0] != f) ++l0;
                while (p.lv_frame[l1] != f) --l1;
            }
            const long long fbase = (long long)fa * per_frame;
            bool beaten = false;
            for (int l = l0; l <= l1 && !beaten; ++l) {
                const LevelDesc d = p.lv[l];
                const int HW = d.rows * d.cols;
                if (HW <= 0) continue;             // a 0 x 0 level has no cells
                const R s = (R)p.scales[l];
                for (int c = 0; c < p.NC && !beaten; ++c) {
                    const PartWalk &root = p.walk[p.walk_off[c]];
                    int kmax = 0;
#pragma unroll
                    for (int m = 0; m < kMaxMix; ++m) kmax = max(kmax, root.ksize[m]);   // unused entries are 0
                    const long long wmax = (long long)round_mul<R>(kmax, s) + 1;         // |round(ks * s) - 1| <= it
                    int wx0, wx1, wy0, wy1;
                    sn_window(xa, wa, wmax, (double)s, d.padx, d.cols, wx0, wx1);
                    sn_window(ya, ha, wmax, (double)s, d.pady, d.rows, wy0, wy1);
                    const int ww = wx1 - wx0, n = ww > 0 && wy1 > wy0 ? ww * (wy1 - wy0) : 0;   // at most HW < 2^31
                    const long long pbase = fbase + d.cell_off * p.NC + (long long)c * HW;
                    for (int e0 = 0; e0 < n; e0 += 64) {
                        const int e = e0 + lane;
                        bool beats = false;
                        if (e < n) {
                            const int y = wy0 + e / ww, x = wx0 + e % ww;
                            const long long ob = pbase + (long long)y * d.cols + x;
                            const R sb = rootv[ob];
                            if (ob != oa && sn_eligible<R>(a, p, ob, sb) && sn_better(sb, ob, sa, oa)) {
                                int xb, yb, wb, hb;
                                sn_root_rect<R>(p, ob, l, c, x, y, xb, yb, wb, hb);
                                beats = sn_covers(xa, ya, wa, ha, xb, yb, wb, hb) || sn_covers(xb, yb, wb, hb, xa, ya, wa, ha);
                            }
                        }
                        if (__ballot(beats) != 0ull) { beaten = true; break; }
                    }
                }
            }
            if (beaten) beaten_set |= 1ull << j;
        }
        // 4. the span's bytes
        if (o < p.ntotal) a.dst[o] = (elig && !((beaten_set >> lane) & 1ull)) ? (uint8_t)255 : (uint8_t)0;
    }
}

// a record that takes part: a frame of the call, a part count in range, a score that is not NaN
__device__ inline bool sn_record_ok(const DcParams &p, const int32_t *r)
{
    const long long f = (long long)r[kRecFrame] - p.frame_offset;
    const int n = r[kRecNparts];
    const float s = __int_as_float(r[kRecScore]);
    return f >= 0 && f < p.nframes && n >= 1 && n <= p.max_parts && s == s;
}

// first record of [0, n) whose frame word is >= f
__device__ inline int sn_frame_bound(const DcParams &p, int n, long long f)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)p.in[1 + (size_t)mid * p.stride + kRecFrame] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kSnThreads) void k_scale_nms_records(DcParams p, int dl)
{
    __shared__ int partial[kSnWaves];
    const int i = blockIdx.x * kSnThreads + threadIdx.x, n = dc_count(p);
    int keep = 0;
    if (i < n) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        if (sn_record_ok(p, r)) {                                   // any other record is dropped and is nobody's neighbour
            const float s = __int_as_float(r[kRecScore]);
            const int32_t *ra = record_part(r, 0);
            const long long la = r[kRecLevel];
            const int lo = sn_frame_bound(p, n, r[kRecFrame]), hi = sn_frame_bound(p, n, (long long)r[kRecFrame] + 1);
            keep = 1;
            for (int o = lo; o < hi && keep; ++o) {
                const int32_t *q = p.in + 1 + (size_t)o * p.stride;
                if (o == i || !sn_record_ok(p, q)) continue;
                const long long d = (long long)q[kRecLevel] - la;
                if (d > dl || d < -(long long)dl || !sn_better(__int_as_float(q[kRecScore]), o, s, i)) continue;
                const int32_t *rb = record_part(q, 0);
                if (sn_covers(ra[0], ra[1], ra[2], ra[3], rb[0], rb[1], rb[2], rb[3]) ||
                    sn_covers(rb[0], rb[1], rb[2], rb[3], ra[0], ra[1], ra[2], ra[3])) keep = 0;
            }
        }
    }
    p.flag[i] = keep;   // [blocks * kSnThreads]
    const int tot = block_sum<kSnWaves, int>(keep, partial);
    if (threadIdx.x == 0) p.blk[blockIdx.x] = tot;
}

}  // namespace

void launch_scale_nms_roots(const ArgminParams &p, const ScaleNmsRoots &a, bool f64, hipStream_t s)
{
    if (p.ntotal <= 0) return;
    const long long nspans = (p.ntotal + 63) / 64;
    const dim3 grid((unsigned)std::max<long long>(std::min<long long>((nspans + kSnWaves - 1) / kSnWaves, kSnMaxGrid), 1));
    if (f64) PBD_LAUNCH(k_scale_nms<double>, grid, dim3(kSnThreads), 0, s, p, a);
    else PBD_LAUNCH(k_scale_nms<float>, grid, dim3(kSnThreads), 0, s, p, a);
}

void launch_scale_nms_records(const DcParams &p, int dl, hipStream_t s)
{
    PBD_LAUNCH(k_scale_nms_records, dim3(dc_record_blocks(p.in_cap)), dim3(kSnThreads), 0, s, p, dl);
    launch_dc_emit(p, s);
}

}  // namespace pbd
