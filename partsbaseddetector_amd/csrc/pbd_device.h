// pbd_device.h (private) -- the device idioms the post-detection stage kernels share, one definition each: the lock-free
// union-find, the wave / workgroup scan, rank and sum, the device-wide exclusive scan, the wave-aggregated atomic add, the
// order-preserving keys, the reduction R(.) of include/pbd.h, and the candidate record's words, hull and count.  The stage files
// (pbd_kernels_cloud / planes / consistency / depth / post / publish / qp / eval / kmeans .hip) keep only what is their own.
// All integer arithmetic here is exact, so a caller's result does not depend on which of these it is built from.
#pragma once

#include "pbd_internal.h"

#include <stddef.h>

#include <type_traits>

namespace pbd {

// ---- constants --------------------------------------------------------------------------------------------------------------
__device__ inline float qnan_f() { return __int_as_float(0x7fc00000); }
__device__ inline double qnan_d() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---- candidate records (include/pbd.h: pbd_candidate_hdr, then nparts boxes of x, y, w, h) ----------------------------------
static_assert(sizeof(pbd_candidate_hdr) == 8 * sizeof(int32_t), "a record's header is eight words");
constexpr int kRecFrame = offsetof(pbd_candidate_hdr, frame) / 4;
constexpr int kRecComponent = offsetof(pbd_candidate_hdr, component) / 4;
constexpr int kRecScore = offsetof(pbd_candidate_hdr, score) / 4;       // float bits
constexpr int kRecNparts = offsetof(pbd_candidate_hdr, nparts) / 4;
constexpr int kRecParts = sizeof(pbd_candidate_hdr) / 4;               // first word of part 0
static_assert(kRecFrame == 0 && kRecComponent == 1 && kRecScore == 5 && kRecNparts == 6 && kRecParts == 8, "record layout");

// part k of record r: x, y, w, h
__device__ inline const int32_t *record_part(const int32_t *r, int k) { return r + kRecParts + 4 * k; }

// records of a device payload (word 0 = the count found, which may exceed the capacity or be a negative status)
__device__ inline int payload_count(const int32_t *in, int in_cap) { return max(min(in[0], in_cap), 0); }
// the list filters (pbd_depth_consistency*, pbd_depth_prune*): a negative or too-large word 0 is no complete list -- no record is
// read and the output's word 0 is -1
__device__ inline bool dc_overflow(const DcParams &p) { return p.in[0] < 0 || p.in[0] > p.in_cap; }
__device__ inline int dc_count(const DcParams &p) { return dc_overflow(p) ? 0 : p.in[0]; }

// cv::Rect operator& in 64 bits (an empty intersection is Rect())
__device__ inline void rect_and64(long long &x, long long &y, long long &w, long long &h, long long bx, long long by, long long bw,
                                  long long bh)
{
    const long long x1 = x > bx ? x : bx, y1 = y > by ? y : by;
    w = (x + w < bx + bw ? x + w : bx + bw) - x1;
    h = (y + h < by + bh ? y + h : by + bh) - y1;
    x = x1; y = y1;
    if (w <= 0 || h <= 0) x = y = w = h = 0;
}

// Candidate::boundingBox (include/Candidate.hpp:105-111): the fold of cv::Rect operator| over the record's parts in member
// order (an empty left side takes the right side as it is, an empty right side is skipped); 64-bit so that x + w cannot wrap
__device__ inline void record_hull64(const int32_t *r, int nparts, long long &x, long long &y, long long &w, long long &h)
{
    x = y = w = h = 0;
    for (int k = 0; k < nparts; ++k) {
        const int32_t *q = record_part(r, k);
        const long long bx = q[0], by = q[1], bw = q[2], bh = q[3];
        if (w <= 0 || h <= 0) {
            x = bx; y = by; w = bw; h = bh;
        } else if (bw > 0 && bh > 0) {
            const long long x1 = min(x, bx), y1 = min(y, by);
            w = max(x + w, bx + bw) - x1;
            h = max(y + h, by + bh) - y1;
            x = x1; y = y1;
        }
    }
}

// first index in the ascending a[0, n) whose element is >= v (T: int32_t or uint32_t)
template <typename T> __device__ inline int lower_bound_i32(const T *a, int n, T v)
{
    static_assert(std::is_integral<T>::value && sizeof(T) == 4, "a table of 32-bit integers");
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- order-preserving integer keys ------------------------------------------------------------------------------------------
// a < b as floats <=> key(a) < key(b) as unsigned integers, for every pair that is not NaN and not {-0, +0} (all bits of a
// negative value flipped, the sign bit of a positive one set); the callers deal with NaN and the zeros first
__device__ inline uint32_t float_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ inline float float_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
__device__ inline unsigned long long double_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double double_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- one wave ---------------------------------------------------------------------------------------------------------------
// the number of set bits of a ballot below this lane: a flagged lane's position among the wave's flagged lanes
__device__ inline int lane_rank(unsigned long long ballot) { return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// inclusive prefix sum over the lanes of the wave
template <typename T> __device__ inline T wave_incl_scan(T x)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// the sum over the lanes of the wave, in every lane
template <typename T> __device__ inline T wave_sum(T x)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// cnt[key] += 1 for every active lane with `on`, one atomic per distinct key of the wave (neighbouring lanes mostly share a
// counter).  cnt is LDS or global memory and key an index into it (>= 0).  Every lane of the wave must make the call (the
// ballots are taken over the wave)
template <typename C> __device__ inline void wave_add_by_key(C *cnt, int key, bool on)
{
    if (!on) key = -1;                                  // no leader's key
    unsigned long long pending = __ballot(on);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lk = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == lk);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(cnt + lk, (C)__popcll(same));
        pending &= ~same;
    }
}

// ---- one workgroup of WAVES waves (lds: WAVES words of the caller's) --------------------------------------------------------
// exclusive prefix of v over the workgroup, and the workgroup's total.  Two barriers: lds may be reused at once
template <typename T, int WAVES> __device__ inline T block_scan(T v, T *lds, T &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T x = wave_incl_scan(v);
    if (lane == 63) lds[w] = x;
    __syncthreads();
    T base = 0, tot = 0;
    for (int k = 0; k < WAVES; ++k) {
        if (k < w) base += lds[k];
        tot += lds[k];
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// the position of a flagged thread among the workgroup's flagged threads, and their number.  Two barriers
template <int WAVES> __device__ inline int block_rank(bool flag, int *lds, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) lds[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < WAVES; ++k) {
        if (k < w) base += lds[k];
        tot += lds[k];
    }
    __syncthreads();
    total = tot;
    return base + lane_rank(m);
}

// the sum of v over the workgroup in every thread, accumulated over the wave sums as A.  ONE barrier, after the write: the caller
// keeps lds untouched until every thread has passed another barrier (or alternates between two lds arrays)
template <int WAVES, typename A, typename T> __device__ inline A block_sum(T v, T *lds)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    A s = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) s += lds[k];
    return s;
}

// ---- the reduction R(.) of include/pbd.h over one workgroup of PBD_QP_LANES threads (pbd_kernels_qp / kmeans .hip) --------------
// The caller's lane-strided partial sums go in; a halving tree per 64 lanes (one wavefront: __shfl_down), then a halving tree
// over the 16 wavefront sums.
constexpr int kRLanes = PBD_QP_LANES;
constexpr int kRWaves = kRLanes / 64;
static_assert(kRLanes == 1024 && kRWaves == 16, "the reduction order of include/pbd.h");

// R(v) of one value per thread; every thread receives the result.  red: 17 doubles of LDS.  Contains two barriers.
__device__ inline double reduce1(double v, double *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h, 64);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (wave == 0) {
        double s = lane < kRWaves ? red[lane] : 0.0;
        for (int h = kRWaves / 2; h >= 1; h >>= 1) s = s + __shfl_down(s, h, 64);
        if (lane == 0) red[kRWaves] = s;
    }
    __syncthreads();
    return red[kRWaves];
}

// two reductions at once: red holds 34 doubles
__device__ inline void reduce2(double u, double v, double *red, double *ru, double *rv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h = 32; h >= 1; h >>= 1) { u = u + __shfl_down(u, h, 64); v = v + __shfl_down(v, h, 64); }
    if (lane == 0) { red[wave] = u; red[kRWaves + 1 + wave] = v; }
    __syncthreads();
    if (wave == 0) {
        double s = lane < kRWaves ? red[lane] : 0.0, t = lane < kRWaves ? red[kRWaves + 1 + lane] : 0.0;
        for (int h = kRWaves / 2; h >= 1; h >>= 1) { s = s + __shfl_down(s, h, 64); t = t + __shfl_down(t, h, 64); }
        if (lane == 0) { red[kRWaves] = s; red[2 * kRWaves + 1] = t; }
    }
    __syncthreads();
    *ru = red[kRWaves];
    *rv = red[2 * kRWaves + 1];
}

// ---- lock-free union-find (ECL-CC style) ------------------------------------------------------------------------------------
// parent[x] <= x always, and a root is the smallest element of its set, so the result does not depend on the order of the
// atomics.  Parents are read and shortened with agent-scope relaxed accesses; only the compare-and-swap on a root hooks.  A stale
// read returns an older ancestor, which delays nothing but speed.
__device__ inline int uf_ld(int32_t *a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void uf_st(int32_t *a, int v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// x's root so far; the path walked is shortened
__device__ inline int uf_find(int32_t *parent, int x)
{
    int cur = uf_ld(parent + x);
    if (cur != x) {
        int next, prev = x;
        while (cur > (next = uf_ld(parent + cur))) {
            uf_st(parent + prev, next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// the root WITHOUT shortening the path, for the kernel that runs after all hooking and writes every element's final root into
// parent[]: a shortening store racing with that write could put back an intermediate ancestor
__device__ inline int uf_root(const int32_t *parent, int x)
{
    int p;
    while ((p = parent[x]) != x) x = p;
    return x;
}

// joins the sets of a and b: the larger root is hooked under the smaller
__device__ inline void uf_unite(int32_t *parent, int a, int b)
{
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        if (ra < rb) {
            const int ret = atomicCAS(parent + rb, rb, ra);
            if (ret == rb) return;
            rb = ret;
        } else {
            const int ret = atomicCAS(parent + ra, ra, rb);
            if (ret == ra) return;
            ra = ret;
        }
    }
}

// ---- device-wide exclusive scan, three launches -----------------------------------------------------------------------------
// a[0, n) of stored type T becomes its exclusive prefix sums and a[n] the total (`copy`, when given, receives the same n + 1
// values): k_scan_part (one sum per tile of kScanTile elements), k_scan_top (one workgroup: the exclusive scan of the tile sums
// in place, part[tiles] = the total, then top(total) by thread 0), k_scan_add (the tiles).  n is *n_dev when n_dev is given
// (a count only the device knows), else n_host.  A is the type the workgroup scans accumulate in; the tile sums are long long.
// The kernels and their launcher live in an unnamed namespace: each stage file gets its own, none is exported.
constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kScanTile = 4 * kScanThreads;

struct ScanNoTop {
    __device__ void operator()(long long) const {}
};

namespace {

template <typename T, typename A>
__global__ __launch_bounds__(kScanThreads) void k_scan_part(const T *a, long long n_host, const long long *n_dev, long long *part)
{
    __shared__ A lds[kScanWaves];
    const long long n = n_dev ? *n_dev : n_host;
    const long long tiles = (n + kScanTile - 1) / kScanTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        A s = 0;
        for (int k = 0; k < 4; ++k) {
            const long long e = t * kScanTile + threadIdx.x * 4 + k;
            if (e < n) s += a[e];
        }
        A total;
        block_scan<A, kScanWaves>(s, lds, total);
        if (threadIdx.x == 0) part[t] = total;
    }
}

template <typename A, typename Top>
__global__ __launch_bounds__(kScanThreads) void k_scan_top(long long *part, long long n_host, const long long *n_dev, Top top)
{
    __shared__ A lds[kScanWaves];
    const long long n = n_dev ? *n_dev : n_host;
    const long long tiles = (n + kScanTile - 1) / kScanTile;
    long long carry = 0;
    for (long long t0 = 0; t0 < tiles; t0 += kScanThreads) {
        const long long t = t0 + threadIdx.x;
        const A v = t < tiles ? (A)part[t] : 0;
        A total;
        const A ex = block_scan<A, kScanWaves>(v, lds, total);
        if (t < tiles) part[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        part[tiles] = carry;
        top(carry);
    }
}

template <typename T, typename A>
__global__ __launch_bounds__(kScanThreads) void k_scan_add(T *a, T *copy, long long n_host, const long long *n_dev,
                                                           const long long *part)
{
    __shared__ A lds[kScanWaves];
    const long long n = n_dev ? *n_dev : n_host;
    const long long tiles = (n + kScanTile - 1) / kScanTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        A v[4], s = 0;
        for (int k = 0; k < 4; ++k) {
            const long long e = t * kScanTile + threadIdx.x * 4 + k;
            v[k] = e < n ? (A)a[e] : 0;
            s += v[k];
        }
        A total;
        A run = (A)part[t] + block_scan<A, kScanWaves>(s, lds, total);
        for (int k = 0; k < 4; ++k) {
            const long long e = t * kScanTile + threadIdx.x * 4 + k;
            if (e < n) {
                a[e] = (T)run;
                if (copy) copy[e] = (T)run;
            }
            run += v[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a[n] = (T)part[tiles];
        if (copy) copy[n] = (T)part[tiles];
    }
}

// `grid` workgroups for the two tile kernels (the caller's cap of ceil(n / kScanTile))
template <typename A, typename T, typename Top>
void launch_scan(T *a, T *copy, long long n_host, const long long *n_dev, long long *part, int grid, Top top, hipStream_t s)
{
    PBD_LAUNCH((k_scan_part<T, A>), dim3(grid), dim3(kScanThreads), 0, s, (const T *)a, n_host, n_dev, part);
    PBD_LAUNCH((k_scan_top<A, Top>), dim3(1), dim3(kScanThreads), 0, s, part, n_host, n_dev, top);
    PBD_LAUNCH((k_scan_add<T, A>), dim3(grid), dim3(kScanThreads), 0, s, a, copy, n_host, n_dev, (const long long *)part);
}

}  // namespace

}  // namespace pbd
