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
#include "pbd_device.h"

#include <algorithm>

namespace pbd {
namespace {

constexpr int kPostThreads = 256;
// the suppression's workgroup: 256 threads over an LDS canvas; 1024 over a global one, whose count loop is bound by the latency
// of its L2 reads (fewer, wider rounds per candidate)
template <bool kLds> constexpr int post_nms_threads() { return kLds ? 256 : 1024; }
constexpr size_t kPostLdsCanvasMax = 128 * 1024;   // bytes of bit canvas held in LDS (160 KiB per CU on gfx950)

__device__ inline bool post_overflow(const PostParams &p) { return p.in[0] > p.in_cap || (p.bad && *p.bad); }
__device__ inline int post_count(const PostParams &p) { return payload_count(p.in, p.in_cap); }

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
    const long long f = (long long)p.in[1 + (size_t)i * p.stride + kRecFrame] - p.in_offset;
    const long long g = i > 0 ? (long long)p.in[1 + (size_t)(i - 1) * p.stride + kRecFrame] - p.in_offset : 0;
    if (f < 0 || f >= p.nframes || f < g) *p.bad = 1;
}

__global__ __launch_bounds__(kPostThreads) void k_post_prep(PostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (post_overflow(p) || i >= post_count(p)) return;
    const int32_t *r = p.in + 1 + (size_t)i * p.stride;
    p.key[i] = __int_as_float(r[kRecScore]);
    const int f = r[kRecFrame] - p.in_offset;
    p.frame[i] = f;
    const int np = min(max(r[kRecNparts], 0), p.max_parts);
    // Candidate::boundingBox & Rect(0, 0, cols, rows), as corners; an empty intersection is (0, 0, 0, 0)
    long long x, y, w, h;
    record_hull64(r, np, x, y, w, h);
    const int2 fs = p.fdim ? p.fdim[f] : make_int2(p.rows, p.cols);   // the frame's own size (mixed-size calls)
    rect_and64(x, y, w, h, 0, 0, fs.y, fs.x);
    p.box[i] = make_int4((int)x, (int)y, (int)(x + w), (int)(y + h));
}

__global__ __launch_bounds__(kPostThreads) void k_post_rank(PostParams p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = post_count(p);
    if (post_overflow(p) || i >= n) return;
    const int f = p.frame[i];
    const int lo = lower_bound_i32(p.frame, n, f), hi = lower_bound_i32(p.frame, n, f + 1);
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
    const int lo = lower_bound_i32(p.frame, n, f), hi = lower_bound_i32(p.frame, n, f + 1);
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
        const int buf = phase & 1;                 // two partial arrays in turn: a suppressed candidate's one barrier is enough
        ++phase;
        const long long boxsum = block_sum<kWaves, long long>(cnt, partial[buf]);
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
    const int lo = lower_bound_i32(p.frame, n, f), hi = lower_bound_i32(p.frame, n, f + 1);
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
