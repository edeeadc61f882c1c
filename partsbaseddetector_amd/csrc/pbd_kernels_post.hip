// pbd_kernels_post.hip -- opt-in per-frame post-processing of the candidate list (pbd_set_nms): what every caller of the
// reference runs after detect() -- Candidate::sort then Candidate::nonMaximaSuppression(im, candidates, overlap)
// (cells/detect.cpp:237-238, ros/Node.cpp:192-196; include/Candidate.hpp:91-99,105-111,277-304).
//
// Input: the argmin payload (word 0 = candidates found, then the records grouped by frame, `frame` field frame-local).
//   k_post_prep   one thread per record: dense score / frame arrays, the part hull clipped to the frame
//   k_post_rank   one thread per record: rank = #(greater score in its frame) + #(equal score, smaller index) -- a stable
//                 descending sort, exact, with -0.0 == +0.0 (float compare, not a bit-pattern key)
//   k_post_nms    one workgroup per frame (256 / 1024 threads): the greedy painted-canvas suppression over a BIT canvas (one bit per pixel, rows
//                 of ceil(cols/32) words), in LDS when it fits, else in a per-frame slice of a global workspace
//   k_post_emit   one workgroup per frame: the kept records, frame by frame, into the output payload
// A found count above the input capacity makes the output's word 0 = -1 (suppression of a truncated list would differ).
#include "pbd_internal.h"

#include <algorithm>

namespace pbd {
namespace {

constexpr int kPostThreads = 256;
// the suppression's workgroup: 256 threads over an LDS canvas; 1024 over a global one, whose count loop is bound by the latency
// of its L2 reads (fewer, wider rounds per candidate)
template <bool kLds> constexpr int post_nms_threads() { return kLds ? 256 : 1024; }
constexpr size_t kPostLdsCanvasMax = 128 * 1024;   // bytes of bit canvas held in LDS (160 KiB per CU on gfx950)

__device__ inline bool post_overflow(const PostParams &p) { return p.in[0] > p.in_cap || (p.bad && *p.bad); }
__device__ inline int post_count(const PostParams &p) { return max(min(p.in[0], p.in_cap), 0); }

// first index in [0, n) whose frame is >= f (the list is grouped by ascending frame)
__device__ inline int post_lower_bound(const int *frame, int n, int f)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (frame[mid] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// does (a, ia) precede (b, ib)?  Descending score, equal scores by index (Python's stable list.sort on key -score).
// NaN scores (never produced by the dynamic program) go last, by index, so that the ranks stay a permutation.
__device__ inline bool post_ahead(float a, int ia, float b, int ib)
{
    const bool an = a != a, bn = b != b;
    if (an != bn) return bn;
    if (!an && a != b) return a > b;
    return ia < ib;
}

// pbd_suppress*: a caller's list is checked first (word 0 >= 0, every frame index in range, grouped ascending)
__global__ __launch_bounds__(kPostThreads) void k_post_check(PostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && p.in[0] < 0) *p.bad = 1;
    if (i >= post_count(p) || p.in[0] > p.in_cap) return;
    const long long f = (long long)p.in[1 + (size_t)i * p.stride] - p.in_offset;
    const long long g = i > 0 ? (long long)p.in[1 + (size_t)(i - 1) * p.stride] - p.in_offset : 0;
    if (f < 0 || f >= p.nframes || f < g) *p.bad = 1;
}

__global__ __launch_bounds__(kPostThreads) void k_post_prep(PostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (post_overflow(p) || i >= post_count(p)) return;
    const int32_t *r = p.in + 1 + (size_t)i * p.stride;
    p.key[i] = __int_as_float(r[5]);
    const int f = r[0] - p.in_offset;
    p.frame[i] = f;
    const int np = min(max(r[6], 0), p.max_parts);
    // Candidate::boundingBox: fold of cv::Rect operator| over the parts (an empty left side takes the right side, an empty
    // right side is skipped); 64-bit so that x + w cannot wrap
    long long x = 0, y = 0, w = 0, h = 0;
    for (int k = 0; k < np; ++k) {
        const long long bx = r[8 + 4 * k], by = r[9 + 4 * k], bw = r[10 + 4 * k], bh = r[11 + 4 * k];
        if (w <= 0 || h <= 0) {
            x = bx; y = by; w = bw; h = bh;
        } else if (bw > 0 && bh > 0) {
            const long long x1 = min(x, bx), y1 = min(y, by);
            w = max(x + w, bx + bw) - x1;
            h = max(y + h, by + bh) - y1;
            x = x1; y = y1;
        }
    }
    // box & Rect(0, 0, cols, rows); an empty intersection is (0, 0, 0, 0)
    const int2 fs = p.fdim ? p.fdim[f] : make_int2(p.rows, p.cols);   // the frame's own size (mixed-size calls)
    long long x1 = max(x, 0LL), y1 = max(y, 0LL), x2 = min(x + w, (long long)fs.y), y2 = min(y + h, (long long)fs.x);
    if (x2 - x1 <= 0 || y2 - y1 <= 0) x1 = y1 = x2 = y2 = 0;
    p.box[i] = make_int4((int)x1, (int)y1, (int)x2, (int)y2);
}

__global__ __launch_bounds__(kPostThreads) void k_post_rank(PostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = post_count(p);
    if (post_overflow(p) || i >= n) return;
    const int f = p.frame[i];
    const int lo = post_lower_bound(p.frame, n, f), hi = post_lower_bound(p.frame, n, f + 1);
    const float ki = p.key[i];
    int rank = 0;
    for (int j = lo; j < hi; ++j) rank += post_ahead(p.key[j], j, ki, i) ? 1 : 0;
    p.perm[lo + rank] = i;
}

// one workgroup per frame; per candidate: popcount of the box's canvas words (edge-masked), workgroup sum, decision, paint.
// Two barriers per painted candidate, one per suppressed one, none for an empty box (kept, nothing painted).
template <bool kLds>
__global__ __launch_bounds__(post_nms_threads<kLds>()) void k_post_nms(PostParams p)
{
    constexpr int NT = post_nms_threads<kLds>(), kWaves = NT / 64, kUnroll = 4;
    extern __shared__ __attribute__((aligned(16))) uint32_t post_lds[];
    __shared__ int partial[2][kWaves];
    const int f = p.flist ? p.flist[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
    if (post_overflow(p)) return;
    const int n = post_count(p);
    const int lo = post_lower_bound(p.frame, n, f), hi = post_lower_bound(p.frame, n, f + 1);
    const int wpr = p.fdim ? (p.fdim[f].y + 31) / 32 : p.wpr;
    const long long words = (long long)(p.fdim ? p.fdim[f].x : p.rows) * wpr;
    uint32_t *canvas = kLds ? post_lds : p.canvas + (p.fcanvas ? (size_t)p.fcanvas[f] : (size_t)f * words);
    for (long long t = tid; t < words; t += NT) canvas[t] = 0u;
    __syncthreads();
    const double overlap = (double)p.overlap;      // the reference's `const float overlap`, widened in the comparison
    int kept = 0, phase = 0;
    for (int k = lo; k < hi; ++k) {
        const int4 b = p.box[p.perm[k]];
        const int bw = b.z - b.x, bh = b.w - b.y;
        if (bw <= 0 || bh <= 0) {                  // area 0: boxsum / area is NaN, NaN > overlap is false -> kept
            if (tid == 0) p.slot[k] = kept;
            ++kept;
            continue;
        }
        const int wx0 = b.x >> 5, wx1 = (b.z - 1) >> 5, nw = wx1 - wx0 + 1;
        const uint32_t lmask = ~0u << (b.x & 31), rmask = ~0u >> (31 - ((b.z - 1) & 31));
        const int total = nw * bh;
        int cnt = 0;
        for (int t0 = tid; t0 < total; t0 += kUnroll * NT) {     // kUnroll independent reads in flight per round
            uint32_t v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int t = t0 + u * NT;
                v[u] = 0u;
                if (t < total) {
                    const int row = t / nw, wi = t - row * nw;
                    uint32_t m = ~0u;
                    if (wi == 0) m &= lmask;
                    if (wi == nw - 1) m &= rmask;
                    v[u] = canvas[(size_t)(b.y + row) * wpr + wx0 + wi] & m;
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) cnt += __popc(v[u]);
        }
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        const int buf = phase & 1;
        ++phase;
        if ((tid & 63) == 0) partial[buf][tid >> 6] = cnt;
        __syncthreads();
        long long boxsum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) boxsum += partial[buf][w];
        const double ratio = (double)boxsum / ((double)bw * (double)bh);
        if (ratio > overlap) {
            if (tid == 0) p.slot[k] = -1;
            continue;                               // nothing painted: the next count may start without a barrier
        }
        for (int t = tid; t < total; t += NT) {   // every word belongs to one thread: plain read-modify-write
            const int row = t / nw, wi = t - row * nw;
            uint32_t m = ~0u;
            if (wi == 0) m &= lmask;
            if (wi == nw - 1) m &= rmask;
            canvas[(size_t)(b.y + row) * wpr + wx0 + wi] |= m;
        }
        if (tid == 0) p.slot[k] = kept;
        ++kept;
        __syncthreads();
    }
    if (tid == 0) p.fkept[f] = kept;
}

__global__ __launch_bounds__(kPostThreads) void k_post_emit(PostParams p)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    if (post_overflow(p)) {
        if (f == 0 && tid == 0) p.out[0] = -1;
        return;
    }
    const int n = post_count(p);
    int off = 0, total = 0;
    for (int g = 0; g < p.nframes; ++g) {
        const int c = p.fkept[g];
        off += g < f ? c : 0;
        total += c;
    }
    if (f == 0 && tid == 0) p.out[0] = total;
    const int lo = post_lower_bound(p.frame, n, f), hi = post_lower_bound(p.frame, n, f + 1);
    const int stride = p.stride;
    const long long words = (long long)(hi - lo) * stride;
    for (long long t = tid; t < words; t += kPostThreads) {
        const int k = lo + (int)(t / stride), w = (int)(t % stride);
        const int s = p.slot[k];
        if (s < 0 || off + s >= p.out_cap) continue;
        int32_t v = p.in[1 + (size_t)p.perm[k] * stride + w];
        if (w == 0) v += p.frame_offset;
        p.out[1 + (size_t)(off + s) * stride + w] = v;
    }
}

}  // namespace

bool post_canvas_in_lds(int rows, int cols)
{
    return (size_t)rows * ((cols + 31) / 32) * sizeof(uint32_t) <= kPostLdsCanvasMax;
}

size_t post_canvas_words(int rows, int cols) { return (size_t)rows * ((cols + 31) / 32); }

void launch_postprocess(const PostParams &p, hipStream_t s)
{
    const int rblocks = std::max((p.in_cap + kPostThreads - 1) / kPostThreads, 1);
    PBD_LAUNCH(k_post_prep, dim3(rblocks), dim3(kPostThreads), 0, s, p);
    PBD_LAUNCH(k_post_rank, dim3(rblocks), dim3(kPostThreads), 0, s, p);
    if (post_canvas_in_lds(p.rows, p.cols)) {
        static const bool lds_limit_set = [] {   // once: the largest canvas held in LDS
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_post_nms<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kPostLdsCanvasMax);
            return true;
        }();
        (void)lds_limit_set;
        const unsigned lds = (unsigned)std::max<size_t>(post_canvas_words(p.rows, p.cols) * sizeof(uint32_t), 16);
        PBD_LAUNCH(k_post_nms<true>, dim3(p.nframes), dim3(post_nms_threads<true>()), lds, s, p);
    } else {
        PBD_LAUNCH(k_post_nms<false>, dim3(p.nframes), dim3(post_nms_threads<false>()), 0, s, p);
    }
    PBD_LAUNCH(k_post_emit, dim3(p.nframes), dim3(kPostThreads), 0, s, p);
}

void launch_postprocess_mixed(const PostParams &p, const int *lds_frames, int nlds, size_t lds_words, const int *glb_frames,
                              int nglb, hipStream_t s)
{
    const int rblocks = std::max((p.in_cap + kPostThreads - 1) / kPostThreads, 1);
    if (p.bad) PBD_LAUNCH(k_post_check, dim3(rblocks), dim3(kPostThreads), 0, s, p);
    PBD_LAUNCH(k_post_prep, dim3(rblocks), dim3(kPostThreads), 0, s, p);
    PBD_LAUNCH(k_post_rank, dim3(rblocks), dim3(kPostThreads), 0, s, p);
    // each frame is suppressed on a canvas of its own kind: one launch over the frames whose canvas fits in LDS, one over the rest
    if (nlds > 0) {
        static const bool lds_limit_set = [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_post_nms<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kPostLdsCanvasMax);
            return true;
        }();
        (void)lds_limit_set;
        PostParams q = p;
        q.flist = lds_frames;
        const unsigned lds = (unsigned)std::max<size_t>(lds_words * sizeof(uint32_t), 16);
        PBD_LAUNCH(k_post_nms<true>, dim3(nlds), dim3(post_nms_threads<true>()), lds, s, q);
    }
    if (nglb > 0) {
        PostParams q = p;
        q.flist = glb_frames;
        PBD_LAUNCH(k_post_nms<false>, dim3(nglb), dim3(post_nms_threads<false>()), 0, s, q);
    }
    PBD_LAUNCH(k_post_emit, dim3(p.nframes), dim3(kPostThreads), 0, s, p);
}

}  // namespace pbd
