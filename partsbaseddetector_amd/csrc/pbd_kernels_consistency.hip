// pbd_kernels_consistency.hip -- opt-in depth consistency of each candidate record (pbd_depth_consistency):
// SearchSpacePruning<T>::filterCandidatesByDepth(parts, candidates, depth, zfactor) (src/SearchSpacePruning.cpp:73-95), the
// step the reference's detect(im, depth) leaves commented out (src/PartsBasedDetector.cpp:91-93).
//
// Every (record, part) median is computed once and read as child and as parent:
//   k_dc_classify   one thread per (record, part): the part box clipped to the depth image; an empty box has no median (NaN),
//                   the others go to their size class's segment of one work list (a counting pass, then a placing pass)
//   k_dc_select     per size class, an exact radix select of the element at rank M / 2 over order-preserving integer keys (8,
//                   16, 32 or 64 bits by depth code and T), one 8-bit digit per pass, 256 LDS counters updated once per distinct
//                   digit of a wave (wave_add_by_key, pbd_device.h):
//                     M <= 1024   one wave per median, the keys loaded once into registers (16 per lane)
//                     M <= 4096   one 256-thread workgroup per median, the keys in registers
//                     larger      one 1024-thread workgroup per median, every pass reading the box of the depth image in place
//   k_dc_decide     one thread per record: the reference's edge test over p = 1 .. nparts-1; per 256 records the kept count
//   k_dc_emit       the kept records, byte for byte, in input order (a stable compaction) into the output payload
// No host synchronisation; the workspace grows with the records (a median and a work-list entry per part), never with the
// samples, and the depth images are read where the caller put them.
#include "pbd_device.h"

#include <algorithm>

namespace pbd {
namespace {

constexpr int kDcThreads = 256;       // classify / decide / emit; also the register class of up to kDcBlockKeys
constexpr int kDcWaves = kDcThreads / 64;
constexpr int kDcKeysPerThread = 16;
constexpr int kDcStreamThreads = 1024;
static_assert(kDcWaveKeys == 64 * kDcKeysPerThread && kDcBlockKeys == kDcThreads * kDcKeysPerThread, "size classes");

// bits of the order-preserving key: 8U / 16U samples are exact in T and ordered as unsigned integers; 32F samples (exact in
// double) and 64F samples rounded to float order as floats; 64F samples of a T = double handle as doubles
template <int D, bool F64> constexpr int dc_key_bits()
{
    return D == kDepth8U ? 8 : D == kDepth16U ? 16 : (D == kDepth64F && F64) ? 64 : 32;
}

// the key of sample x of `row` as T: NaN reads as 0, -0.0 as +0.0 (x + 0 is +0 for both zeros, a no-op otherwise)
template <int D, bool F64> __device__ inline unsigned long long dc_key(const uint8_t *row, int x)
{
    if (D == kDepth8U) return row[x];
    if (D == kDepth16U) return reinterpret_cast<const uint16_t *>(row)[x];
    if (D == kDepth64F && F64) {
        double v = reinterpret_cast<const double *>(row)[x];
        return double_key(v != v ? 0.0 : __dadd_rn(v, 0.0));
    }
    float v = D == kDepth32F ? reinterpret_cast<const float *>(row)[x] : (float)reinterpret_cast<const double *>(row)[x];
    return float_key(v != v ? 0.f : __fadd_rn(v, 0.f));
}

// the median as a double (exact for every T)
template <int D, bool F64> __device__ inline double dc_unkey(unsigned long long k)
{
    if (D == kDepth8U || D == kDepth16U) return (double)k;
    if (D == kDepth64F && F64) return double_unkey(k);
    return (double)float_unkey((uint32_t)k);
}

// a record of this call: frame index in range, a known component, nparts its component's part count (1..max parts)
__device__ inline bool dc_record(const DcParams &p, const int32_t *r, int *frame, int *p0, int *np)
{
    const long long f = (long long)r[kRecFrame] - p.frame_offset;
    const int c = r[kRecComponent];
    if (f < 0 || f >= p.nframes || c < 0 || c >= p.NC) return false;
    const int n = r[kRecNparts];
    if (n < 1 || n > p.max_parts || n != p.part_offset[c + 1] - p.part_offset[c]) return false;
    *frame = (int)f; *p0 = p.part_offset[c]; *np = n;
    return true;
}

// part j of record r clipped to the depth image (cv::Rect operator& in 64 bits): x, y, w, h
__device__ inline int4 dc_box(const int32_t *r, int j, const Box3dFrame &fr)
{
    const int32_t *q = record_part(r, j);
    long long x = q[0], y = q[1], w = q[2], h = q[3];
    rect_and64(x, y, w, h, 0, 0, fr.cols, fr.rows);
    return make_int4((int)x, (int)y, (int)w, (int)h);
}

// the start of class k's segment of the one work list: the classes before it, counted by the first pass
__device__ inline int dc_seg(const DcParams &p, int k) { return (k > 0 ? p.qn[0] : 0) + (k > 1 ? p.qn[1] : 0); }

// kPlace = false: counts the tasks of each class (qn[0..2]); kPlace = true: writes each task into its class's segment (cursors
// qn[3..5]).  Two passes over the tasks keep the work list at one entry per (record, part).
template <bool kPlace>
__global__ __launch_bounds__(kDcThreads) void k_dc_classify(DcParams p)
{
    const int n = dc_count(p), lane = threadIdx.x & 63;
    const long long ntask = (long long)n * p.max_parts;
    // every lane of a wave runs the same iterations: the work-list slots are taken with one atomic per class and wave
    for (long long t0 = (long long)blockIdx.x * kDcThreads; t0 < ntask; t0 += (long long)gridDim.x * kDcThreads) {
        const long long t = t0 + threadIdx.x;
        int cls = -1;
        if (t < ntask) {
            const int i = (int)(t / p.max_parts), j = (int)(t - (long long)i * p.max_parts);
            const int32_t *r = p.in + 1 + (size_t)i * p.stride;
            int f, p0, np;
            if (dc_record(p, r, &f, &p0, &np) && np >= 2 && j < np) {   // else no median is read (a one-part component keeps)
                const int4 b = dc_box(r, j, p.frames[f]);
                const long long M = (long long)b.z * b.w;
                if (M == 0) { if (!kPlace) p.med[t] = qnan_d(); }   // no median
                else cls = M <= kDcWaveKeys ? 0 : M <= kDcBlockKeys ? 1 : 2;
            }
        }
        for (int k = 0; k < 3; ++k) {
            const unsigned long long m = __ballot(cls == k);
            if (!m) continue;
            const int leader = __ffsll((long long)m) - 1;
            if (!kPlace) {
                if (lane == leader) atomicAdd(&p.qn[k], __popcll(m));
                continue;
            }
            int base = 0;
            if (lane == leader) base = atomicAdd(&p.qn[3 + k], __popcll(m));
            base = __shfl(base, leader, 64);
            if (cls == k) p.queue[dc_seg(p, k) + base + lane_rank(m)] = (int)t;
        }
    }
}

struct DcSelShared {
    uint32_t hist[256];
    unsigned int digit, rem;
};

// the key at rank `rank` of the keys `each` visits (each(fn) calls fn(key, valid) the same number of times in every lane of a
// wave): KBITS / 8 passes, the bits above the pass's digit fixed by the passes before
template <int NT, int KBITS, class Each>
__device__ unsigned long long dc_select(DcSelShared &S, unsigned int rank, Each each)
{
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long prefix = 0;
    unsigned int rem = rank;
    for (int shift = KBITS - 8; shift >= 0; shift -= 8) {
        for (int t = tid; t < 256; t += NT) S.hist[t] = 0;
        __syncthreads();
        const int hs = shift + 8;
        each([&](unsigned long long k, bool valid) {
            const bool match = valid && (hs >= KBITS || (k >> hs) == (prefix >> hs));
            wave_add_by_key(S.hist, (int)((k >> shift) & 255), match);
        });
        __syncthreads();
        if (tid < 64) {   // wave 0: the bin in which the remaining rank falls (4 bins per lane, a wave prefix sum)
            const uint32_t c0 = S.hist[4 * lane], c1 = S.hist[4 * lane + 1], c2 = S.hist[4 * lane + 2], c3 = S.hist[4 * lane + 3];
            const unsigned int s = c0 + c1 + c2 + c3;
            const unsigned int incl = wave_incl_scan(s);
            const unsigned int excl = incl - s;
            if (excl <= rem && rem < incl) {
                unsigned int r = rem - excl;
                int d = 4 * lane;
                if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
                S.digit = (unsigned int)d;
                S.rem = r;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)S.digit << shift;
        rem = S.rem;
        __syncthreads();
    }
    return prefix;
}

// the register classes: NT threads per median, kDcKeysPerThread keys each, loaded once
template <int D, bool F64, int NT>
__global__ __launch_bounds__(NT) void k_dc_select_regs(DcParams p, int cls)
{
    constexpr int KB = dc_key_bits<D, F64>();
    __shared__ DcSelShared S;
    const int tid = threadIdx.x;
    const int count = p.qn[cls];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int t = p.queue[dc_seg(p, cls) + q];
        const int i = t / p.max_parts, j = t - i * p.max_parts;
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        const Box3dFrame fr = p.frames[r[kRecFrame] - p.frame_offset];
        const int4 b = dc_box(r, j, fr);
        const int M = b.z * b.w;
        unsigned long long key[kDcKeysPerThread];
#pragma unroll
        for (int k = 0; k < kDcKeysPerThread; ++k) {
            const int e = tid + k * NT;
            key[k] = 0;
            if (e < M) {
                const int y = e / b.z, x = e - y * b.z;
                key[k] = dc_key<D, F64>(fr.data + (size_t)(b.y + y) * (size_t)fr.pitch, b.x + x);
            }
        }
        const unsigned long long m = dc_select<NT, KB>(S, (unsigned int)(M / 2), [&](auto fn) {
#pragma unroll
            for (int k = 0; k < kDcKeysPerThread; ++k) fn(key[k], tid + k * NT < M);
        });
        if (tid == 0) p.med[t] = dc_unkey<D, F64>(m);
    }
}

// the streaming class: every pass reads the box in place, a wave per row, a lane per column
template <int D, bool F64>
__global__ __launch_bounds__(kDcStreamThreads) void k_dc_select_stream(DcParams p)
{
    constexpr int KB = dc_key_bits<D, F64>(), kWaves = kDcStreamThreads / 64;
    __shared__ DcSelShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = p.qn[2];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int t = p.queue[dc_seg(p, 2) + q];
        const int i = t / p.max_parts, j = t - i * p.max_parts;
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        const Box3dFrame fr = p.frames[r[kRecFrame] - p.frame_offset];
        const int4 b = dc_box(r, j, fr);
        const long long M = (long long)b.z * b.w;
        const unsigned long long m = dc_select<kDcStreamThreads, KB>(S, (unsigned int)(M / 2), [&](auto fn) {
            for (int y = wave; y < b.w; y += kWaves) {
                const uint8_t *row = fr.data + (size_t)(b.y + y) * (size_t)fr.pitch;
                for (int x0 = 0; x0 < b.z; x0 += 64) {
                    const int x = x0 + lane;
                    fn(x < b.z ? dc_key<D, F64>(row, b.x + x) : 0ull, x < b.z);
                }
            }
        });
        if (tid == 0) p.med[t] = dc_unkey<D, F64>(m);
    }
}

// (double)std::abs(mc - mq) in T: float T rounds the difference to float
template <bool F64> __device__ inline double dc_absdiff(double a, double b)
{
    if (F64) return fabs(__dsub_rn(a, b));
    return (double)fabsf(__fsub_rn((float)a, (float)b));
}

template <bool F64>
__global__ __launch_bounds__(kDcThreads) void k_dc_decide(DcParams p)
{
    __shared__ int partial[kDcWaves];
    const int i = blockIdx.x * kDcThreads + threadIdx.x;
    const int n = dc_count(p);
    int keep = 0;
    if (i < n) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        int f, p0, np;
        if (dc_record(p, r, &f, &p0, &np)) {
            keep = 1;
            const double thr_z = (double)p.zfactor;
            const double *med = p.med + (size_t)i * p.max_parts;
            for (int c = 1; c < np && keep; ++c) {
                const int par = p.parent[p0 + c];
                const double mc = med[c], mq = med[par];
                if (mc != mc || mq != mq) continue;           // an empty box: no median, no test
                if (!(mc > 0 && mq > 0)) continue;
                const double d = dc_absdiff<F64>(mc, mq);     // Inf - Inf is NaN: the comparison is false
                if (d > __dmul_rn(p.norm[p0 + c], thr_z)) keep = 0;
            }
        }
    }
    p.flag[i] = keep;   // [blocks * kDcThreads]
    const int tot = block_sum<kDcWaves, int>(keep, partial);
    if (threadIdx.x == 0) p.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kDcThreads) void k_dc_emit(DcParams p)
{
    __shared__ int dest[kDcThreads];
    __shared__ int wsum[kDcWaves], wtot[kDcWaves];
    __shared__ int base_s, total_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (dc_overflow(p)) {   // a suppression overflow or a truncated list: no complete list to filter
        if (blockIdx.x == 0 && tid == 0) p.out[0] = -1;
        return;
    }
    // kept records before this block, and in all
    int before = 0, total = 0;
    for (int b = tid; b < (int)gridDim.x; b += kDcThreads) {
        const int c = p.blk[b];
        total += c;
        before += b < (int)blockIdx.x ? c : 0;
    }
    before = wave_sum(before);
    total = wave_sum(total);
    if (lane == 0) { wsum[wave] = before; wtot[wave] = total; }
    __syncthreads();
    if (tid == 0) {
        int s = 0, t = 0;
        for (int w = 0; w < kDcWaves; ++w) { s += wsum[w]; t += wtot[w]; }
        base_s = s;
        total_s = t;
    }
    __syncthreads();   // also ends tid 0's reads of wsum: the scan below writes it
    total = total_s;
    const int i = blockIdx.x * kDcThreads + tid;
    const int n = dc_count(p);
    const int keep = i < n ? p.flag[i] : 0;
    int nkeep;
    const int pos = base_s + block_scan<int, kDcWaves>(keep, wsum, nkeep);
    dest[tid] = keep && pos < p.out_cap ? pos : -1;
    if (blockIdx.x == 0 && tid == 0) p.out[0] = total;
    __syncthreads();
    const int stride = p.stride;
    const int nrec = min(kDcThreads, max(n - (int)blockIdx.x * kDcThreads, 0));
    for (int w = tid; w < nrec * stride; w += kDcThreads) {
        const int k = w / stride, o = w - k * stride;
        const int d = dest[k];
        if (d >= 0) p.out[1 + (size_t)d * stride + o] = p.in[1 + (size_t)(blockIdx.x * kDcThreads + k) * stride + o];
    }
}

template <int D, bool F64>
void launch_dc_select(const DcParams &p, int ntask, hipStream_t s)
{
    const int g0 = std::max(std::min(ntask, kDcMaxGrid * 4), 1), g1 = std::max(std::min(ntask, kDcMaxGrid), 1);
    const int g2 = std::max(std::min(ntask, kDcMaxGrid / 4), 1);
    PBD_LAUNCH((k_dc_select_regs<D, F64, 64>), dim3(g0), dim3(64), 0, s, p, 0);
    PBD_LAUNCH((k_dc_select_regs<D, F64, kDcThreads>), dim3(g1), dim3(kDcThreads), 0, s, p, 1);
    PBD_LAUNCH((k_dc_select_stream<D, F64>), dim3(g2), dim3(kDcStreamThreads), 0, s, p);
}

template <bool F64>
void launch_dc_select_t(const DcParams &p, int ntask, hipStream_t s)
{
    switch (p.depth) {
    case kDepth8U: launch_dc_select<kDepth8U, F64>(p, ntask, s); break;
    case kDepth16U: launch_dc_select<kDepth16U, F64>(p, ntask, s); break;
    case kDepth32F: launch_dc_select<kDepth32F, F64>(p, ntask, s); break;
    default: launch_dc_select<kDepth64F, F64>(p, ntask, s); break;
    }
}

}  // namespace

int dc_record_blocks(int in_cap) { return std::max((in_cap + kDcThreads - 1) / kDcThreads, 1); }

void launch_dc_emit(const DcParams &p, hipStream_t s)
{
    PBD_LAUNCH(k_dc_emit, dim3(dc_record_blocks(p.in_cap)), dim3(kDcThreads), 0, s, p);
}

void launch_depth_consistency(const DcParams &p, bool f64, int step, hipStream_t s)
{
    const long long ntask = (long long)std::max(p.in_cap, 0) * p.max_parts;
    switch (step) {
    case kDcStepClassify: {
        const int grid = (int)std::max<long long>(std::min<long long>((ntask + kDcThreads - 1) / kDcThreads, kDcMaxGrid), 1);
        PBD_LAUNCH(k_dc_classify<false>, dim3(grid), dim3(kDcThreads), 0, s, p);
        PBD_LAUNCH(k_dc_classify<true>, dim3(grid), dim3(kDcThreads), 0, s, p);
        break;
    }
    case kDcStepSelect:
        if (f64) launch_dc_select_t<true>(p, (int)std::min<long long>(ntask, 1 << 30), s);
        else launch_dc_select_t<false>(p, (int)std::min<long long>(ntask, 1 << 30), s);
        break;
    default: {
        const int blocks = dc_record_blocks(p.in_cap);
        if (f64) PBD_LAUNCH(k_dc_decide<true>, dim3(blocks), dim3(kDcThreads), 0, s, p);
        else PBD_LAUNCH(k_dc_decide<false>, dim3(blocks), dim3(kDcThreads), 0, s, p);
        launch_dc_emit(p, s);
        break;
    }
    }
}

}  // namespace pbd
