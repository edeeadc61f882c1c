// pbd_kernels_topk.hip -- opt-in exact selection of the K best elements of every segment of a packed array (pbd_top_k_cells*,
// pbd_set_top_k) and of every frame of a candidate list (pbd_top_k*).  The rule is stated in include/pbd.h: a is better than b when
// its value is larger, or equal and its index smaller; NaN and masked elements take no part.
//
// Cells: a most-significant-digit radix select on the order-preserving keys of pbd_device.h (-0.0 canonicalised to +0.0 first),
// 8 bits per pass, 4 passes for float and 8 for double whatever the data.  Every segment is cut into tiles of kTkTile elements of
// its own, so a workgroup always works for one segment; the tiles of all segments form one list the grid strides over.
//   k_topk_hist<R, Elig>   pass p: the digit p of every eligible element whose higher digits equal the segment's prefix, counted
//                          in an LDS histogram (tk_add_digit), then one integer atomic per non-empty bin into hist[seg][256]
//   k_topk_pick            one wave per segment: the digit that holds the K-th best (a suffix sum over the 256 bins), the new
//                          prefix and the number still to take inside it; the bins are zeroed for the next pass.  Pass 0 also
//                          settles K = 0 (nothing) and K >= eligible (everything)
//   k_topk_ties<R, Elig>   after the last pass the prefix is the pivot key and `need` the pivot-valued elements to keep: their
//                          number per tile; launch_scan (pbd_device.h) turns it into the exclusive prefix over the tiles
//   k_topk_mark<R, Elig>   dst = 255 where key > pivot, or key == pivot and the element's rank among the segment's pivot-valued
//                          elements in index order is below `need`; 0 elsewhere.  Every byte of dst is written
// All counts are integers, so the atomics' order changes nothing, and ties are decided by the scan alone: two runs agree byte for
// byte.  The work per element is the same for every input: no pass is skipped and nothing is compacted.
//
// Records: k_topk_records, one thread per record, counts the better records of its own frame (the list is grouped by ascending
// frame, so the frame is a range found by bisection) and keeps the record when fewer than K are; the depth-consistency filter's
// compaction (launch_dc_emit) writes the kept ones in input order.  Its cost depends on the frames' record counts only.
#include "pbd_device.h"

#include <algorithm>
#include <limits.h>

namespace pbd {
namespace {

constexpr int kTkThreads = 256;
constexpr int kTkWaves = kTkThreads / 64;
constexpr int kTkRows = kTkTile / kTkThreads;   // elements per thread of a tile, kTkThreads apart
constexpr int kTkMaxGrid = 4096;
static_assert(kTkTile % kTkThreads == 0 && kTkThreads == 256, "one thread per histogram bin, whole rows per tile");

struct TkAll {
    template <typename R> __device__ bool operator()(R v, size_t) const { return v == v; }
};
struct TkMask {
    const uint8_t *mask;
    template <typename R> __device__ bool operator()(R v, size_t i) const { return v == v && mask[i] != 0; }
};
// the detect path: the find's own expression (NaN compares false) and the bytes of the filters before this one
template <typename R> struct TkAbove {
    R thresh;
    const uint8_t *ok, *mx;
    __device__ bool operator()(R v, size_t i) const { return v > thresh && (!ok || ok[i] != 0) && (!mx || mx[i] != 0); }
};

// the order-preserving key of a value that is not NaN; the two zeros share one
__device__ inline uint32_t tk_key(float v) { return float_key(v == 0.f ? 0.f : v); }
__device__ inline unsigned long long tk_key(double v) { return double_key(v == 0.0 ? 0.0 : v); }
template <typename R> struct TkKey { typedef uint32_t type; };
template <> struct TkKey<double> { typedef unsigned long long type; };

// bins[digit] += 1 for every lane with `on`, digit in 0..255: eight ballots give each lane the lanes that share its digit, and the
// first of them adds their number -- one LDS atomic instruction per call, its lanes on different addresses, whatever the digits
// are.  (wave_add_by_key loops once per distinct key of the wave: a pass over 256 evenly spread digits cost 1.7 times a pass over
// a few, profiles/top_k/README.md.)  Every lane of the wave must make the call
__device__ inline void tk_add_digit(int *bins, int digit, bool on)
{
    unsigned long long peers = __ballot(on);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    if (on && (int)(threadIdx.x & 63) == __ffsll((long long)peers) - 1) atomicAdd(bins + digit, (int)__popcll(peers));
}

// the segment of tile t and the tile's place in it
struct TkWhere {
    int seg;
    long long tile_in_seg, tile0;   // tile0: the segment's first tile
    long long off, len;             // the segment's first element and length
};
__device__ inline TkWhere tk_where(const TopKParams &p, long long t)
{
    TkWhere w;
    if (!p.tab) {
        w.seg = (int)(t / p.utiles);
        w.tile0 = (long long)w.seg * p.utiles;
        w.off = (long long)w.seg * p.ulen; w.len = p.ulen;
    } else {
        int lo = 0, hi = p.nseg;                         // the last segment whose first tile is <= t (a segment without
        while (hi - lo > 1) {                            // elements shares its successor's and is skipped)
            const int mid = (lo + hi) >> 1;
            if (p.tab[mid].tile0 <= t) lo = mid; else hi = mid;
        }
        w.seg = lo;
        w.tile0 = p.tab[lo].tile0;
        w.off = p.tab[lo].off; w.len = p.tab[lo + 1].off - w.off;
    }
    w.tile_in_seg = t - w.tile0;
    return w;
}

template <typename R, class Elig>
__global__ __launch_bounds__(kTkThreads) void k_topk_hist(TopKParams p, Elig elig, int pass)
{
    typedef typename TkKey<R>::type Key;
    __shared__ int bins[256];
    const R *src = static_cast<const R *>(p.src);
    const int shift = (int)sizeof(Key) * 8 - 8 * (pass + 1);
    for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const TkWhere w = tk_where(p, t);
        const Key prefix = pass ? (Key)p.state[w.seg].prefix : 0;
        bins[threadIdx.x] = 0;
        __syncthreads();
        for (int j = 0; j < kTkRows; ++j) {
            const long long i = w.tile_in_seg * kTkTile + j * kTkThreads + threadIdx.x;
            bool on = false;
            int digit = 0;
            if (i < w.len) {
                const size_t e = (size_t)(w.off + i);
                const R v = src[e];
                if (elig(v, e)) {
                    const Key key = tk_key(v);
                    on = pass == 0 || (key >> (shift + 8)) == prefix;
                    digit = (int)((key >> shift) & 255);
                }
            }
            tk_add_digit(bins, digit, on);
        }
        __syncthreads();
        const int c = bins[threadIdx.x];
        if (c) atomicAdd(p.hist + (size_t)w.seg * 256 + threadIdx.x, c);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kTkThreads) void k_topk_pick(TopKParams p, int pass)
{
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * kTkWaves;
    for (long long seg = (long long)blockIdx.x * kTkWaves + (threadIdx.x >> 6); seg < p.nseg; seg += nwaves) {
        int *bins = p.hist + (size_t)seg * 256 + 4 * lane;
        int c[4];
        for (int j = 0; j < 4; ++j) { c[j] = bins[j]; bins[j] = 0; }
        TopKSeg st{0ull, p.k, 0, 0};
        if (pass) st = p.state[seg];
        const int s = c[0] + c[1] + c[2] + c[3];
        const int incl = wave_incl_scan(s), total = __shfl(incl, 63, 64);
        if (pass == 0 && (p.k == 0 || total <= p.k)) {
            // nothing: no key is above the largest one and none of its own is taken; everything: every key is >= 0
            st = p.k == 0 ? TopKSeg{~0ull, 0, 1, 0} : TopKSeg{0ull, INT_MAX, 1, 0};
            if (lane == 0) p.state[seg] = st;
        }
        if (st.done) continue;
        int above = total - incl;                        // the elements in the bins of the lanes above this one
        for (int j = 3; j >= 0; --j) {                   // exactly one bin of one lane holds the st.need-th best
            if (st.need > above && st.need <= above + c[j])
                p.state[seg] = TopKSeg{(st.prefix << 8) | (unsigned long long)(4 * lane + j), st.need - above, 0, 0};
            above += c[j];
        }
    }
}

template <typename R, class Elig>
__global__ __launch_bounds__(kTkThreads) void k_topk_ties(TopKParams p, Elig elig)
{
    typedef typename TkKey<R>::type Key;
    __shared__ int lds[kTkWaves];
    const R *src = static_cast<const R *>(p.src);
    for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const TkWhere w = tk_where(p, t);
        const Key pivot = (Key)p.state[w.seg].prefix;
        int n = 0;
        for (int j = 0; j < kTkRows; ++j) {
            const long long i = w.tile_in_seg * kTkTile + j * kTkThreads + threadIdx.x;
            if (i < w.len) {
                const size_t e = (size_t)(w.off + i);
                const R v = src[e];
                n += (elig(v, e) && tk_key(v) == pivot) ? 1 : 0;
            }
        }
        const int tot = block_sum<kTkWaves, int>(n, lds);
        if (threadIdx.x == 0) p.tcnt[t] = tot;
        __syncthreads();
    }
}

template <typename R, class Elig>
__global__ __launch_bounds__(kTkThreads) void k_topk_mark(TopKParams p, Elig elig)
{
    typedef typename TkKey<R>::type Key;
    __shared__ int lds[kTkWaves];
    const R *src = static_cast<const R *>(p.src);
    for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const TkWhere w = tk_where(p, t);
        const TopKSeg st = p.state[w.seg];
        const Key pivot = (Key)st.prefix;
        int before = p.tcnt[t] - p.tcnt[w.tile0];         // the segment's pivot-valued elements in the tiles before this one
        for (int j = 0; j < kTkRows; ++j) {
            const long long i = w.tile_in_seg * kTkTile + j * kTkThreads + threadIdx.x;
            bool ok = false, tie = false, above = false;
            size_t e = 0;
            if (i < w.len) {
                e = (size_t)(w.off + i);
                const R v = src[e];
                ok = elig(v, e);
                if (ok) {
                    const Key key = tk_key(v);
                    above = key > pivot;
                    tie = key == pivot;
                }
            }
            int tot;
            const int rank = before + block_rank<kTkWaves>(tie, lds, tot);
            before += tot;
            if (i < w.len) p.dst[e] = (above || (tie && rank < st.need)) ? (uint8_t)255 : (uint8_t)0;
        }
    }
}

// a record that takes part: a frame of the call, a part count in range, a score that is not NaN
__device__ inline bool tk_record_ok(const DcParams &p, const int32_t *r)
{
    const long long f = (long long)r[kRecFrame] - p.frame_offset;
    const int n = r[kRecNparts];
    const float s = __int_as_float(r[kRecScore]);
    return f >= 0 && f < p.nframes && n >= 1 && n <= p.max_parts && s == s;
}

// first record of [0, n) whose frame word is >= f
__device__ inline int tk_frame_bound(const DcParams &p, int n, long long f)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)p.in[1 + (size_t)mid * p.stride + kRecFrame] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kTkThreads) void k_topk_records(DcParams p, int k)
{
    __shared__ int partial[kTkWaves];
    const int i = blockIdx.x * kTkThreads + threadIdx.x, n = dc_count(p);
    int keep = 0;
    if (i < n) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        if (tk_record_ok(p, r)) {                                   // any other record is dropped
            const float s = __int_as_float(r[kRecScore]);
            const int lo = tk_frame_bound(p, n, r[kRecFrame]), hi = tk_frame_bound(p, n, (long long)r[kRecFrame] + 1);
            int better = 0;
            for (int o = lo; o < hi; ++o) {
                const int32_t *q = p.in + 1 + (size_t)o * p.stride;
                const float t = __int_as_float(q[kRecScore]);
                better += (tk_record_ok(p, q) && (t > s || (t == s && o < i))) ? 1 : 0;
            }
            keep = better < k ? 1 : 0;
        }
    }
    p.flag[i] = keep;   // [blocks * kTkThreads]
    const int tot = block_sum<kTkWaves, int>(keep, partial);
    if (threadIdx.x == 0) p.blk[blockIdx.x] = tot;
}

template <typename R, class Elig> void tk_run(const TopKParams &p, const Elig &elig, hipStream_t s)
{
    const int grid = (int)std::min<long long>(p.ntiles, kTkMaxGrid);
    const int pick = (int)std::min<long long>(((long long)p.nseg + kTkWaves - 1) / kTkWaves, kTkMaxGrid);
    const int passes = (int)sizeof(typename TkKey<R>::type);
    for (int pass = 0; pass < passes; ++pass) {
        PBD_LAUNCH((k_topk_hist<R, Elig>), dim3(grid), dim3(kTkThreads), 0, s, p, elig, pass);
        PBD_LAUNCH(k_topk_pick, dim3(pick), dim3(kTkThreads), 0, s, p, pass);
    }
    PBD_LAUNCH((k_topk_ties<R, Elig>), dim3(grid), dim3(kTkThreads), 0, s, p, elig);
    const int sgrid = (int)std::min<long long>((p.ntiles + kScanTile - 1) / kScanTile, kTkMaxGrid);
    launch_scan<int>(p.tcnt, (int *)nullptr, p.ntiles, nullptr, p.part, sgrid, ScanNoTop{}, s);
    PBD_LAUNCH((k_topk_mark<R, Elig>), dim3(grid), dim3(kTkThreads), 0, s, p, elig);
}

}  // namespace

long long top_k_scan_parts(long long ntiles) { return (ntiles + kScanTile - 1) / kScanTile + 1; }

void launch_top_k(const TopKParams &p, bool f64, hipStream_t s)
{
    if (p.ntiles <= 0 || p.nseg <= 0) return;
    auto run = [&](auto r) {
        using R = decltype(r);
        if (p.use_thresh) tk_run<R>(p, TkAbove<R>{(R)p.thresh, p.mask, p.mask2}, s);
        else if (p.mask) tk_run<R>(p, TkMask{p.mask}, s);
        else tk_run<R>(p, TkAll{}, s);
    };
    if (f64) run(double{}); else run(float{});
}

void launch_top_k_records(const DcParams &p, int k, hipStream_t s)
{
    PBD_LAUNCH(k_topk_records, dim3(dc_record_blocks(p.in_cap)), dim3(kTkThreads), 0, s, p, k);
    launch_dc_emit(p, s);
}

}  // namespace pbd
