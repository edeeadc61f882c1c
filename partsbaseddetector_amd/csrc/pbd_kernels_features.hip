// pbd_kernels_features.hip -- pyramid resampling and HOG feature kernels (gfx950).
//
// Replaces HOGFeatures<T>::pyramid / features<uint8_t> (reference src/HOGFeatures.cpp:95-341) for
// T=float.  All arithmetic is ordered exactly as the reference's; the file is compiled with
// -ffp-contract=off so no multiply-add is fused.
//
// Every per-pixel operation is stated once, as a device function; the kernels differ in how a thread finds its pixel
// (Frames / Runs below), in how many pixels a lane takes and in where the results go.
#include "pbd_internal.h"
#include "pbd_resample.h"

#include <stdlib.h>

#include <type_traits>

namespace pbd {

// ------------------------------------------------------------------------------------------------
// Where a thread works.  The flat index of a launch runs over the elements (OFF: 0 image pixels, 1 blocks, 2 cells) of a
// range of levels; the level comes from a search of the levels' offsets, (y, x) from the level's width.
// ------------------------------------------------------------------------------------------------
template <int OFF>
__device__ __forceinline__ long long lv_off(const LevelDesc &d)
{
    return OFF == 0 ? d.img_off : (OFF == 1 ? d.blk_off : d.cell_off);
}
template <int OFF>
__device__ __forceinline__ int lv_width(const LevelDesc &d)
{
    return OFF == 0 ? d.img_cols : (OFF == 1 ? d.blk_cols : d.cols);
}

// largest i in [lo, hi) with off[i] <= idx  (offsets are non-decreasing)
template <typename Off>
__device__ __forceinline__ int last_not_above(int lo, int hi, long long idx, Off off)
{
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off(mid) <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

// Block-cooperative search, every thread of the block must call it: the candidate offsets go to LDS in ONE memory round
// trip and the search runs there.  (The per-thread search in global memory is six DEPENDENT loads -- ~4000 cycles before a
// wave's first useful instruction -- and was what bounded these short kernels.)  A mixed-size call's virtual frame may hold
// more levels, and its first launch more runs, than the LDS table: those search global memory (uniform branch).
template <typename Off>
__device__ __forceinline__ int last_not_above_blk(int lo, int hi, long long idx, Off off)
{
    __shared__ long long s_off[PBD_MAX_LEVELS];
    if (hi > PBD_MAX_LEVELS) return last_not_above(lo, hi, idx, off);
    for (int i = lo + (int)threadIdx.x; i < hi; i += (int)blockDim.x) s_off[i] = off(i);
    __syncthreads();
    return last_not_above(lo, hi, idx, [&](int i) { return s_off[i]; });
}

// level of [lo, hi) containing flat element `idx`
template <int OFF>
__device__ __forceinline__ int find_level_blk(const LevelDesc *lv, int lo, int hi, long long idx)
{
    return last_not_above_blk(lo, hi, idx, [&](int i) { return lv_off<OFF>(lv[i]); });
}

// the level's descriptor and the element's (y, x) inside it
struct LevelCell {
    LevelDesc d;
    int y, x;
};
template <int OFF>
__device__ __forceinline__ LevelCell level_cell(const LevelDesc *lv, int l, long long idx)
{
    LevelCell c;
    c.d = lv[l];
    const int local = (int)(idx - lv_off<OFF>(c.d));
    c.y = local / lv_width<OFF>(c.d);
    c.x = local - c.y * lv_width<OFF>(c.d);
    return c;
}

// A pixel of a pyramid level under construction, and what it is computed from.
struct SrcImage {               // a caller's frame or region: pitch in bytes
    const uint8_t *base;
    int rows, cols;
    long long pitch;
};
template <typename PT> __device__ __forceinline__ const PT *src_row(const SrcImage &im, int y)
{
    return reinterpret_cast<const PT *>(im.base + (size_t)y * im.pitch);
}
template <typename PT>
struct Site {
    LevelDesc d;                // the level
    int l, y, x;                // its index, the pixel inside it
    PT *dst;                    // the pixel in the pyramid buffer
    SrcImage src;               // resized levels: the image the level is sampled from
    const PT *down;             // pyrDown levels: the image of the source level d.src_level, ...
    int down_rows, down_cols;   // ... its size
};

// Equal-size calls: grid row = frame of the launch, flat index + base = pixel offset in the frame's pyramid, over the levels
// [first, last); the source is the dense frame, a frame's pyramid starts at pixel frame * pix_per_frame.
struct Frames {
    int first, last;
    long long base, npix;
    __device__ __forceinline__ int search(const PyrParams &p, long long idx) const { return find_level_blk<0>(p.lv, first, last, idx + base); }
    __device__ __forceinline__ int level(const PyrParams &, int k) const { return k; }
    __device__ __forceinline__ int local(const PyrParams &, int, long long idx, const LevelDesc &d) const { return (int)(idx + base - d.img_off); }
    __device__ __forceinline__ size_t pix0(const PyrParams &p) const { return (size_t)(p.frame0 + blockIdx.y) * p.pix_per_frame; }
    __device__ __forceinline__ SrcImage source(const PyrParams &p, int, int px_bytes) const
    {
        return SrcImage{p.frames + (size_t)(p.frame0 + blockIdx.y) * p.rows * p.cols * px_bytes, p.rows, p.cols, (long long)p.cols * px_bytes};
    }
};

// Mixed-size calls (pbd_detect_frames*): the levels of the virtual frame come from different source frames.  The launch's
// levels are runs of the flat index (run k = level run_lev[k], pixels [run_off[k], run_off[k + 1])); a resized level reads
// its own frame (pointer, size, pitch: FrameDesc), with the per-frame tables its LevelDesc points into; one pyramid.
struct Runs {
    long long npix;             // run_off[nruns]
    __device__ __forceinline__ int search(const PyrParams &p, long long idx) const
    {
        return last_not_above_blk(0, p.nruns, idx, [&](int i) { return p.run_off[i]; });
    }
    __device__ __forceinline__ int level(const PyrParams &p, int k) const { return p.run_lev[k]; }
    __device__ __forceinline__ int local(const PyrParams &p, int k, long long idx, const LevelDesc &) const { return (int)(idx - p.run_off[k]); }
    __device__ __forceinline__ size_t pix0(const PyrParams &) const { return 0; }
    __device__ __forceinline__ SrcImage source(const PyrParams &p, int l, int) const
    {
        const FrameDesc fr = p.fd[p.lv_frame[l]];
        return SrcImage{fr.data, fr.rows, fr.cols, fr.pitch};
    }
};

// the site of flat pixel idx in the search's result k (a level or a run) ...
template <typename PT, typename Where>
__device__ __forceinline__ void site_at(const PyrParams &p, const Where &w, int k, long long idx, Site<PT> &s)
{
    s.l = w.level(p, k);
    s.d = p.lv[s.l];
    const int local = w.local(p, k, idx, s.d);
    s.y = local / s.d.img_cols; s.x = local - s.y * s.d.img_cols;
    s.dst = reinterpret_cast<PT *>(p.pyr) + (w.pix0(p) + s.d.img_off + local) * p.cn;
}
// ... and of flat pixel idx, false past the launch's last pixel; every thread of the block must call it
template <typename PT, typename Where>
__device__ __forceinline__ bool locate(const PyrParams &p, const Where &w, long long idx, Site<PT> &s)
{
    const int k = w.search(p, idx);
    if (idx >= w.npix) return false;
    site_at(p, w, k, idx, s);
    return true;
}
template <typename PT, typename Where>
__device__ __forceinline__ void locate_down(const PyrParams &p, const Where &w, Site<PT> &s)
{
    const LevelDesc sd = p.lv[s.d.src_level];
    s.down = reinterpret_cast<const PT *>(p.pyr) + (w.pix0(p) + sd.img_off) * p.cn;
    s.down_rows = sd.img_rows; s.down_cols = sd.img_cols;
}

// for_depth, the packed BGR pixel loads and the per-channel operations of cv::resize INTER_LINEAR (resize_fix for 8-bit,
// resize_typed for 16U / 32F / 64F): pbd_resample.h, shared with the warped positives.

// a packed BGR pixel; the last pixel of the source (frame or region) is read bytewise: its 4th byte may lie past the image
// (S0, S1: its rows ty.y0, ty.y1; rows x cols: its size)
__device__ __forceinline__ uint32_t resize_px3(const uint8_t *S0, const uint8_t *S1, int rows, int cols, const ResizeTabY &ty, const ResizeTabX &tx)
{
    auto ld = [&](const uint8_t *row, int yy, int xx) {
        return (yy == rows - 1 && xx == cols - 1) ? load_px3_bytes(row + xx * 3) : load_px3(row + xx * 3);
    };
    const int sx = tx.sx, sx1 = sx + 1 < cols ? sx + 1 : sx;
    const uint32_t p00 = ld(S0, ty.y0, sx), p10 = ld(S1, ty.y1, sx), p01 = ld(S0, ty.y0, sx1), p11 = ld(S1, ty.y1, sx1);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out |= (uint32_t)(uint8_t)resize_fix(px_ch(p00, c), px_ch(p01, c), px_ch(p10, c), px_ch(p11, c), tx, ty) << (8 * c);
    return out;
}

// One thread per destination pixel of the resized levels.
template <typename PT, typename Where>
__global__ __launch_bounds__(256) void k_resize(PyrParams p, Where w)
{
    Site<PT> s;
    if (!locate(p, w, (long long)blockIdx.x * blockDim.x + threadIdx.x, s)) return;
    s.src = w.source(p, s.l, p.cn * (int)sizeof(PT));
    const int cn = p.cn;
    if constexpr (std::is_same<PT, uint8_t>::value) {
        const ResizeTabX tx = p.tabx[s.d.tab_x + s.x];
        const ResizeTabY ty = p.taby[s.d.tab_y + s.y];
        const uint8_t *S0 = src_row<uint8_t>(s.src, ty.y0), *S1 = src_row<uint8_t>(s.src, ty.y1);
        if (cn == 3) {
            const uint32_t v = resize_px3(S0, S1, s.src.rows, s.src.cols, ty, tx);
#pragma unroll
            for (int c = 0; c < 3; ++c) s.dst[c] = (uint8_t)px_ch(v, c);
            return;
        }
        const int sx = tx.sx * cn, sx1 = (tx.sx + 1 < s.src.cols ? tx.sx + 1 : tx.sx) * cn;
        for (int c = 0; c < cn; ++c) s.dst[c] = (uint8_t)resize_fix(S0[sx + c], S0[sx1 + c], S1[sx + c], S1[sx1 + c], tx, ty);
    } else {
        const ResizeTabXf tx = p.tabxf[s.d.tab_x + s.x];
        const ResizeTabYf ty = p.tabyf[s.d.tab_y + s.y];
        const PT *S0 = src_row<PT>(s.src, ty.y0), *S1 = src_row<PT>(s.src, ty.y1);
        for (int c = 0; c < cn; ++c) s.dst[c] = resize_typed<PT>(S0, S1, cn, c, tx, ty);
    }
}

// Four consecutive destination pixels per thread (8-bit BGR frames of one size, the hot case): the 12 result bytes leave as
// three 4-byte stores instead of twelve 1-byte ones and the row coefficients are fetched once.  Quads that run over the end
// of a level row fall back to pixel-by-pixel byte stores.
__global__ __launch_bounds__(256) void k_resize4(PyrParams p, long long npix)
{
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int l = find_level_blk<0>(p.lv, 0, p.interval, min(idx, npix - 1));
    if (idx >= npix) return;
    const int frame = p.frame0 + blockIdx.y;
    const LevelDesc d = p.lv[l];
    const int local = (int)(idx - d.img_off);
    const int dy = local / d.img_cols, dx = local - dy * d.img_cols;
    const uint8_t *src = p.frames + (size_t)frame * p.rows * p.cols * 3;
    uint8_t *D = p.pyr + ((size_t)frame * p.pix_per_frame + idx) * 3;
    if (dx + 3 < d.img_cols) {
        const ResizeTabY ty = p.taby[d.tab_y + dy];
        const uint8_t *S0 = src + (size_t)ty.y0 * p.cols * 3, *S1 = src + (size_t)ty.y1 * p.cols * 3;
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = resize_px3(S0, S1, p.rows, p.cols, ty, p.tabx[d.tab_x + dx + i]);
        u32_unaligned *o = reinterpret_cast<u32_unaligned *>(D);
        o[0] = q[0] | (q[1] << 24);
        o[1] = (q[1] >> 8) | (q[2] << 16);
        o[2] = (q[2] >> 16) | (q[3] << 8);
        return;
    }
    for (int i = 0; i < 4; ++i) {     // the quad wraps to the next row or runs into the next level
        const long long pi = idx + i;
        if (pi >= npix) return;
        int li = l;
        while (li + 1 < p.interval && p.lv[li + 1].img_off <= pi) ++li;
        const LevelDesc di = p.lv[li];
        const int loc = (int)(pi - di.img_off);
        const int y = loc / di.img_cols, x = loc - y * di.img_cols;
        const ResizeTabY ty = p.taby[di.tab_y + y];
        const uint32_t v = resize_px3(src + (size_t)ty.y0 * p.cols * 3, src + (size_t)ty.y1 * p.cols * 3, p.rows, p.cols, ty, p.tabx[di.tab_x + x]);
        D[3 * i] = (uint8_t)v; D[3 * i + 1] = (uint8_t)(v >> 8); D[3 * i + 2] = (uint8_t)(v >> 16);
    }
}

void launch_resize(const PyrParams &p, int nframes, long long npix, hipStream_t s)
{
    if (p.depth == kDepth8U && p.cn == 3) {
        dim3 grid4((unsigned)((npix + 1023) / 1024), nframes);
        PBD_LAUNCH(k_resize4, grid4, dim3(256), 0, s, p, npix);
        return;
    }
    dim3 grid((unsigned)((npix + 255) / 256), nframes);
    for_depth(p.depth, [&](auto t) { PBD_LAUNCH((k_resize<decltype(t), Frames>), grid, dim3(256), 0, s, p, Frames{0, p.interval, 0, npix}); });
}

void launch_resize_runs(const PyrParams &p, hipStream_t s)
{
    const long long npix = p.pix_per_frame;   // run_off[nruns] of this launch
    if (p.nruns == 0 || npix == 0) return;
    dim3 grid((unsigned)((npix + 255) / 256));
    for_depth(p.depth, [&](auto t) { PBD_LAUNCH((k_resize<decltype(t), Runs>), grid, dim3(256), 0, s, p, Runs{npix}); });
}

// ------------------------------------------------------------------------------------------------
// cv::pyrDown (call site src/HOGFeatures.cpp:122): [1 4 6 4 1] x [1 4 6 4 1], BORDER_REFLECT_101.
// 8U / 16U in int, (sum + 128) >> 8; 32F / 64F the same taps in the pixel type, row = s2*6 + (s1+s3)*4 + s0 + s4,
// dst = (r2*6 + (r1+r3)*4 + r0 + r4) * (1/256).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int p, int len)
{
    // the taps reach at most two positions outside [0, len): for len >= 3 one reflection each way is the whole loop, as
    // selects (the loop form cost a compare-and-branch pair per coordinate, ten per pixel)
    if (len >= 3) {
        p = p < 0 ? -p : p;
        return p >= len ? 2 * len - 2 - p : p;
    }
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

template <typename PT> struct PyrWork { typedef PT type; };
template <> struct PyrWork<uint8_t> { typedef int type; };
template <> struct PyrWork<uint16_t> { typedef int type; };
template <typename F> __device__ __forceinline__ auto pyr_taps(F s) { return s(2) * 6 + (s(1) + s(3)) * 4 + s(0) + s(4); }   // s(i): tap i
__device__ __forceinline__ int pyr_finish(int v) { return (v + 128) >> 8; }
__device__ __forceinline__ float pyr_finish(float v) { return v * (1.f / 256.f); }
__device__ __forceinline__ double pyr_finish(double v) { return v * (1. / 256.); }

// destination pixel (y, x) from the source level image S (rows x cols x cn) into D
template <typename PT>
__device__ __forceinline__ void pyrdown_pixel(const PT *S, int rows, int cols, int cn, int y, int x, PT *D)
{
    typedef typename PyrWork<PT>::type WT;
    int xs[5], ys[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        xs[k] = reflect101(2 * x - 2 + k, cols) * cn;
        ys[k] = reflect101(2 * y - 2 + k, rows);
    }
    if constexpr (std::is_same<PT, uint8_t>::value) if (cn == 3) {
        int r[5][3];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint8_t *R = S + (size_t)ys[k] * cols * 3;
            uint32_t q[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) q[i] = load_px3(R + xs[i]);      // source levels live in the pyramid buffer (slack at its end)
#pragma unroll
            for (int c = 0; c < 3; ++c) r[k][c] = pyr_taps([&](int i) { return px_ch(q[i], c); });
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) D[c] = (uint8_t)pyr_finish(pyr_taps([&](int k) { return r[k][c]; }));
        return;
    }
    for (int c = 0; c < cn; ++c) {
        WT r[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const PT *R = S + (size_t)ys[k] * cols * cn + c;
            r[k] = pyr_taps([&](int i) { return (WT)R[xs[i]]; });
        }
        D[c] = (PT)pyr_finish(pyr_taps([&](int k) { return r[k]; }));
    }
}

// One thread per destination pixel of the launch's levels, whose sources are the levels `interval` below.
template <typename PT, typename Where>
__global__ __launch_bounds__(256) void k_pyrdown(PyrParams p, Where w)
{
    Site<PT> s;
    if (!locate(p, w, (long long)blockIdx.x * blockDim.x + threadIdx.x, s)) return;
    locate_down(p, w, s);
    pyrdown_pixel<PT>(s.down, s.down_rows, s.down_cols, p.cn, s.y, s.x, s.dst);
}

// The hot instantiation (8-bit frames of one size) keeps its body written out, with the shared taps and finish: through the Site
// and pyrdown_pixel the same statements compile to other instructions (four more SGPRs, byte extracts for sub-dword selects)
// and the kernel runs 2 % slower (profiles/refactor_features/README.md).
template <>
__global__ __launch_bounds__(256) void k_pyrdown<uint8_t, Frames>(PyrParams p, Frames w)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = find_level_blk<0>(p.lv, w.first, w.last, idx + w.base);
    if (idx >= w.npix) return;
    const int frame = p.frame0 + blockIdx.y;
    const LevelDesc d = p.lv[l];
    const LevelDesc sd = p.lv[d.src_level];
    const int local = (int)(idx + w.base - d.img_off);
    const int y = local / d.img_cols, x = local - y * d.img_cols;
    const int cn = p.cn;
    const uint8_t *S = p.pyr + ((size_t)frame * p.pix_per_frame + sd.img_off) * cn;
    uint8_t *D = p.pyr + ((size_t)frame * p.pix_per_frame + d.img_off + local) * cn;
    int xs[5], ys[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        xs[k] = reflect101(2 * x - 2 + k, sd.img_cols) * cn;
        ys[k] = reflect101(2 * y - 2 + k, sd.img_rows);
    }
    if (cn == 3) {
        int r[5][3];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint8_t *R = S + (size_t)ys[k] * sd.img_cols * 3;
            uint32_t q[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) q[i] = load_px3(R + xs[i]);      // source levels live in the pyramid buffer (slack at its end)
#pragma unroll
            for (int c = 0; c < 3; ++c) r[k][c] = pyr_taps([&](int i) { return px_ch(q[i], c); });
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) D[c] = (uint8_t)pyr_finish(pyr_taps([&](int k) { return r[k][c]; }));
        return;
    }
    for (int c = 0; c < cn; ++c) {
        int r[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint8_t *R = S + (size_t)ys[k] * sd.img_cols * cn + c;
            r[k] = pyr_taps([&](int i) { return (int)R[xs[i]]; });
        }
        D[c] = (uint8_t)pyr_finish(pyr_taps([&](int k) { return r[k]; }));
    }
}

void launch_pyrdown_range(const PyrParams &p, int nframes, int first_level, int last_level, long long base,
                          long long npix, hipStream_t s)
{
    dim3 grid((unsigned)((npix + 255) / 256), nframes);
    const Frames w{first_level, last_level, base, npix};
    for_depth(p.depth, [&](auto t) { PBD_LAUNCH((k_pyrdown<decltype(t), Frames>), grid, dim3(256), 0, s, p, w); });
}

void launch_pyrdown_runs(const PyrParams &p, hipStream_t s)
{
    const long long npix = p.pix_per_frame;   // run_off[nruns] of this launch
    if (p.nruns == 0 || npix == 0) return;
    dim3 grid((unsigned)((npix + 255) / 256));
    for_depth(p.depth, [&](auto t) { PBD_LAUNCH((k_pyrdown<decltype(t), Runs>), grid, dim3(256), 0, s, p, Runs{npix}); });
}

// ------------------------------------------------------------------------------------------------
// HOG gradients: per image pixel, the snapped orientation (0..17) and the gradient magnitude of the strongest
// colour channel (src/HOGFeatures.cpp:205-260; R = reference template parameter T).
// ------------------------------------------------------------------------------------------------
template <typename R> __device__ __forceinline__ R real_sqrt(R v);
template <> __device__ __forceinline__ float real_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double real_sqrt<double>(double v) { return sqrt(v); }

// The difference of two pixels is taken in the pixel type (integers promote to int, float / double subtract as such) and
// then converted to T (features<uint8_t|uint16_t|float|double>, src/HOGFeatures.cpp:136-146).
template <typename R, typename PT> __device__ __forceinline__ R pix_diff(PT a, PT b)
{
    if constexpr (std::is_integral<PT>::value) return (R)((int)a - (int)b);
    else return (R)(a - b);
}

// src/HOGFeatures.cpp:217-237: the strongest channel, third channel first, then G, then B, each only on strictly larger
template <typename R>
__device__ __forceinline__ void hog_pick(R dxb, R dyb, R dxg, R dyg, R dxr, R dyr, R &dx, R &dy, R &v)
{
    const R vb = dxb * dxb + dyb * dyb;
    const R vg = dxg * dxg + dyg * dyg;
    dx = dxr; dy = dyr;
    v = dx * dx + dy * dy;
    if (vg > v) { v = vg; dx = dxg; dy = dyg; }
    if (vb > v) { v = vb; dx = dxb; dy = dyb; }
}

// src/HOGFeatures.cpp:239-250: 18-way orientation snap
template <typename R>
__device__ __forceinline__ int hog_snap(R dx, R dy)
{
    const R uu[9] = {(R)1.000, (R)0.9397, (R)0.7660, (R)0.5000, (R)0.1736, (R)-0.1736, (R)-0.5000, (R)-0.7660, (R)-0.9397};
    const R vv[9] = {(R)0.000, (R)0.3420, (R)0.6428, (R)0.8660, (R)0.9848, (R)0.9848, (R)0.8660, (R)0.6428, (R)0.3420};
    // The reference's scan, k ascending: "if (dot > best) {best = dot; o = k} else if (-dot > best) {best = -dot; o = k + 9}".
    // best is never negative, so at most one of the two tests can pass and the pair is "|dot| > best" with the sign of dot
    // choosing k or k + 9 (a NaN fails every test in both forms).  The tables are antisymmetric / symmetric about k = 4.5
    // (uu[9-j] = -uu[j], vv[9-j] = vv[j]) and rounding is sign-symmetric, so uu[9-j]*dx + vv[9-j]*dy is, bit for bit,
    // vv[j]*dy - uu[j]*dx: eight products and eight sums instead of eighteen and nine; uu[0]*dx + vv[0]*dy is 1*dx + 0*dy.
    R dots[9];
    dots[0] = uu[0] * dx + vv[0] * dy;
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
        const R pa = uu[j] * dx, pb = vv[j] * dy;
        dots[j] = pa + pb;
        dots[9 - j] = pb - pa;
    }
    R best_dot = (R)0;
    int best_o = 0;
    if constexpr (sizeof(R) == 4) {
        // the winner is carried as k | sign bit of its dot product: one and-or per candidate, the k + 9 resolved at the end
        unsigned code = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float ad = __builtin_fabsf(dots[k]);
            const bool win = ad > best_dot;
            code = win ? ((__float_as_uint(dots[k]) & 0x80000000u) | (unsigned)k) : code;
            best_dot = win ? ad : best_dot;
        }
        best_o = (int)(code & 0xfu) + ((code >> 31) ? 9 : 0);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const R dot = dots[k];
            const R ad = dot < (R)0 ? -dot : dot;
            if (ad > best_dot) { best_dot = ad; best_o = dot < (R)0 ? k + 9 : k; }
        }
    }
    return best_o;
}

template <typename R>
__device__ __forceinline__ void hog_grad_pixel(R dxb, R dyb, R dxg, R dyg, R dxr, R dyr, R &mag, int &ori)
{
    R dx, dy, v;
    hog_pick<R>(dxb, dyb, dxg, dyg, dxr, dyr, dx, dy, v);
    ori = hog_snap<R>(dx, dy);
    mag = real_sqrt<R>(v);
}

// interior pixel s of a three-channel image (stride elements per row); 8-bit pixels come in as one 32-bit load each
template <typename R, typename PT>
__device__ __forceinline__ void hog_grad_px3(const PT *s, size_t stride, R &mag, int &ori)
{
    R dx[3], dy[3];
    if constexpr (std::is_same<PT, uint8_t>::value) {
        const uint32_t pd = load_px3(s + stride), pu = load_px3(s - stride), pr = load_px3(s + 3), pl = load_px3(s - 3);
#pragma unroll
        for (int c = 0; c < 3; ++c) { dx[c] = (R)(px_ch(pr, c) - px_ch(pl, c)); dy[c] = (R)(px_ch(pd, c) - px_ch(pu, c)); }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { dx[c] = pix_diff<R, PT>(s[3 + c], *(s - 3 + c)); dy[c] = pix_diff<R, PT>(s[c + stride], *(s + c - stride)); }
    }
    hog_grad_pixel<R>(dx[0], dy[0], dx[1], dy[1], dx[2], dy[2], mag, ori);
}

// Pass 1 of the two-pass form, one thread per image pixel.  Every pixel feeds four blocks, so this part is done once
// per pixel instead of once per (pixel, block).
template <typename R, typename PT>
__global__ __launch_bounds__(256) void k_hog_grad(HogParams p)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = find_level_blk<0>(p.lv, 0, p.nlevels, idx);
    if (idx >= p.pix_per_frame) return;
    const int frame = p.frame0 + blockIdx.y;
    const LevelCell c = level_cell<0>(p.lv, l, idx);
    const int rows = c.d.img_rows, cols = c.d.img_cols, ys = c.y, xs = c.x;
    const size_t o = (size_t)frame * p.pix_per_frame + idx;
    if (xs < 1 || ys < 1 || xs > cols - 2 || ys > rows - 2) return;     // never sampled (clamped to cols-2 / rows-2)
    const int cn = p.cn;
    const PT *im = reinterpret_cast<const PT *>(p.pyr) + ((size_t)frame * p.pix_per_frame + c.d.img_off) * cn;
    const size_t stride = (size_t)cols * cn;
    R mag;
    int ori;
    if (cn == 1) {
        const PT *s = im + xs + (size_t)ys * stride;
        const R dy = pix_diff<R, PT>(s[stride], *(s - stride));
        const R dx = pix_diff<R, PT>(s[1], s[-1]);
        ori = hog_snap<R>(dx, dy);
        mag = real_sqrt<R>(dx * dx + dy * dy);
    } else hog_grad_px3<R, PT>(im + 3 * xs + (size_t)ys * stride, stride, mag, ori);
    static_cast<R *>(p.gmag)[o] = mag;
    p.gori[o] = (uint8_t)ori;
}

// Four consecutive interior pixels of one row of an 8-bit BGR image, s the first: the rows above / below come in as one
// 16-byte load each and the row itself as 16 + 4 bytes (10 memory instructions per four pixels instead of 24 with results),
// the results are packed for one 16-byte and one 4-byte store.
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ int px_byte(const u32x4_u &v, uint32_t extra, int b)
{   // byte b (compile-time) of the 20 bytes {v, extra}
    const uint32_t w = b < 16 ? v[b >> 2] : extra;
    return (int)((w >> (8 * (b & 3))) & 0xffu);
}
__device__ __forceinline__ void hog_grad_quad(const uint8_t *s, size_t stride, f32x4_u &mg, uint32_t &og)
{
    const u32x4_u up = *reinterpret_cast<const u32x4_u *>(s - stride), dn = *reinterpret_cast<const u32x4_u *>(s + stride);
    const u32x4_u mid = *reinterpret_cast<const u32x4_u *>(s - 3);
    const uint32_t mid2 = *reinterpret_cast<const u32_unaligned *>(s + 13);       // bytes 16..19 of the row window
    og = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // pixel i: up / down at bytes 3i+c, left at window bytes 3i+c, right at 3(i+2)+c
        float m; int oo;
        hog_grad_pixel<float>((float)(px_byte(mid, mid2, 3 * (i + 2) + 0) - px_byte(mid, mid2, 3 * i + 0)),
                              (float)(px_byte(dn, 0, 3 * i + 0) - px_byte(up, 0, 3 * i + 0)),
                              (float)(px_byte(mid, mid2, 3 * (i + 2) + 1) - px_byte(mid, mid2, 3 * i + 1)),
                              (float)(px_byte(dn, 0, 3 * i + 1) - px_byte(up, 0, 3 * i + 1)),
                              (float)(px_byte(mid, mid2, 3 * (i + 2) + 2) - px_byte(mid, mid2, 3 * i + 2)),
                              (float)(px_byte(dn, 0, 3 * i + 2) - px_byte(up, 0, 3 * i + 2)), m, oo);
        mg[i] = m;
        og |= (uint32_t)oo << (8 * i);
    }
}

// Pass 1, four consecutive pixels per thread (8-bit BGR, T = float): quads that share an image row and are all interior take
// hog_grad_quad, the others go pixel by pixel.
__global__ __launch_bounds__(256) void k_hog_grad4(HogParams p)
{
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int l = find_level_blk<0>(p.lv, 0, p.nlevels, min(idx, p.pix_per_frame - 1));
    if (idx >= p.pix_per_frame) return;
    const int frame = p.frame0 + blockIdx.y;
    const LevelCell c = level_cell<0>(p.lv, l, idx);
    const int rows = c.d.img_rows, cols = c.d.img_cols, ys = c.y, xs = c.x;
    const size_t o = (size_t)frame * p.pix_per_frame + idx;
    float *gmag = static_cast<float *>(p.gmag);
    const bool fast = ys * cols + xs + 3 < rows * cols && xs >= 1 && xs + 3 <= cols - 2 && ys >= 1 && ys <= rows - 2;
    if (fast) {
        const uint8_t *im = p.pyr + ((size_t)frame * p.pix_per_frame + c.d.img_off) * 3;
        const size_t stride = (size_t)cols * 3;
        f32x4_u mg;
        uint32_t og;
        hog_grad_quad(im + 3 * xs + (size_t)ys * stride, stride, mg, og);
        *reinterpret_cast<f32x4_u *>(gmag + o) = mg;
        *reinterpret_cast<u32_unaligned *>(p.gori + o) = og;
        return;
    }
    // quads that touch an image border, wrap to the next row or cross into the next level: pixel by pixel
    for (int i = 0; i < 4; ++i) {
        const long long pi = idx + i;
        if (pi >= p.pix_per_frame) return;
        int li = l;
        while (li + 1 < p.nlevels && p.lv[li + 1].img_off <= pi) ++li;
        const LevelCell ci = level_cell<0>(p.lv, li, pi);
        const int r2 = ci.d.img_rows, c2 = ci.d.img_cols, y = ci.y, x = ci.x;
        if (x < 1 || y < 1 || x > c2 - 2 || y > r2 - 2) continue;     // never sampled (clamped to cols-2 / rows-2)
        const uint8_t *im = p.pyr + ((size_t)frame * p.pix_per_frame + ci.d.img_off) * 3;
        const size_t stride = (size_t)c2 * 3;
        float m; int oo;
        hog_grad_px3<float, uint8_t>(im + 3 * x + (size_t)y * stride, stride, m, oo);
        gmag[(size_t)frame * p.pix_per_frame + pi] = m;
        p.gori[(size_t)frame * p.pix_per_frame + pi] = (uint8_t)oo;
    }
}

// ------------------------------------------------------------------------------------------------
// HOG cell histograms, gather form.  One thread per block (cell of the `blocks` grid): it walks the source pixels that
// the reference's scatter loop (src/HOGFeatures.cpp:202-267) adds into this block, in the same raster order, and adds
// (wy*wx)*mag into the bin of the pixel's orientation, so every bin sees the same sequence of additions.  The 18 bins of a
// thread live in LDS ([18][BS], BS threads: the thread always hits bank tid % 32), so the update is one read-add-write
// instead of 18 predicated register adds.
// ------------------------------------------------------------------------------------------------
// pixels with ip in {b-1, b}: (y+0.5)/sbin - 0.5 in [b-1, b+1), i.e. y in [sbin*b - sbin/2 - 0.5, sbin*b + 3*sbin/2 - 0.5);
// one extra pixel either side, the table test of the walk decides
struct HogWindow { int ylo, yhi, xlo, xhi; };
__device__ __forceinline__ HogWindow hog_window(int sbin, int by, int bx, int vish, int visw)
{
    HogWindow w;
    w.ylo = sbin * by - (sbin + 1) / 2 - 1; w.yhi = sbin * by + (3 * sbin + 1) / 2 + 1;
    w.xlo = sbin * bx - (sbin + 1) / 2 - 1; w.xhi = sbin * bx + (3 * sbin + 1) / 2 + 1;
    if (w.ylo < 1) w.ylo = 1;
    if (w.xlo < 1) w.xlo = 1;
    if (w.yhi > vish - 1) w.yhi = vish - 1;
    if (w.xhi > visw - 1) w.xhi = visw - 1;
    return w;
}

// where the walk reads magnitude and orientation of image position (y, x): the planes of pass 1 ...
template <typename R>
struct HogPlanes {
    const R *mag;
    const uint8_t *ori;
    int cols;
    __device__ __forceinline__ int col(int x) const { return x; }
    __device__ __forceinline__ size_t row(int y) const { return (size_t)y * cols; }
    __device__ __forceinline__ R mag_at(size_t g) const { return mag[g]; }
    __device__ __forceinline__ int ori_at(size_t g) const { return (int)ori[g]; }
};
// ... or a workgroup's LDS tile, LW cells per row, cell (0, 0) = image position (oy, ox)
template <int LW>
struct HogLdsTile {
    const float *mag;
    const uint8_t *ori;
    int oy, ox;
    __device__ __forceinline__ int col(int x) const { return x - ox; }
    __device__ __forceinline__ int row(int y) const { return (y - oy) * LW; }
    __device__ __forceinline__ float mag_at(int g) const { return mag[g]; }
    __device__ __forceinline__ int ori_at(int g) const { return (int)ori[g]; }
};

// The walk for a compile-time sbin SB: the x weights of the thread's window are fetched once into registers instead of once
// per source pixel (the coordinate-table loads were most of the kernel's memory requests: lanes are blocks, their table
// entries sbin apart).  h: the thread's bins, BS apart.
template <typename R, int SB, int BS, typename Src>
__device__ __forceinline__ void hog_walk(const HogCoordT<R> *coord, const HogWindow &w, int by, int bx, int rows, int cols, const Src &src, R *h)
{
    constexpr int NX = 2 * SB + 2;                         // window width before clamping
    const int x0 = SB * bx - (SB + 1) / 2 - 1;
    R wxs[NX];
    int xoff[NX];                                           // source column, -1: this x does not feed the block
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const int x = x0 + i;
        xoff[i] = -1; wxs[i] = (R)0;
        if (x >= w.xlo && x < w.xhi) {
            const HogCoordT<R> cx = coord[x];
            if (cx.ip == bx) { wxs[i] = cx.v1; xoff[i] = src.col(x < cols - 2 ? x : cols - 2); }            // this block is (., ixp): weight vx1
            else if (cx.ip + 1 == bx) { wxs[i] = cx.v0; xoff[i] = src.col(x < cols - 2 ? x : cols - 2); }   // (., ixp+1): weight vx0
        }
    }
    for (int y = w.ylo; y < w.yhi; ++y) {
        const HogCoordT<R> cy = coord[y];
        R wy;
        if (cy.ip == by) wy = cy.v1;
        else if (cy.ip + 1 == by) wy = cy.v0;
        else continue;
        const auto rowg = src.row(y < rows - 2 ? y : rows - 2);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            if (xoff[i] < 0) continue;
            const auto g = rowg + xoff[i];
            const R contrib = (wy * wxs[i]) * src.mag_at(g);
            R *bin = h + src.ori_at(g) * BS;
            *bin = *bin + contrib;
        }
    }
}

// the block's 18 bins and its energy (src/HOGFeatures.cpp:270-283)
template <typename R, int BS>
__device__ __forceinline__ void hog_hist_store(const R *h, R *hist, R *norm, long long blk_per_frame)
{
    R hv[18];
#pragma unroll
    for (int o = 0; o < 18; ++o) { hv[o] = h[o * BS]; hist[(size_t)o * blk_per_frame] = hv[o]; }
    R e = (R)0;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const R t = hv[o] + hv[o + 9];
        e += t * t;
    }
    *norm = e;
}

// Pass 2 of the two-pass form.  SB = compile-time sbin (4, 8) or 0 for any.  RANGE: the launch covers the blocks [p.blk0, p.blk1)
// of the levels [p.lv0, p.lv1) -- one bin size of a plan that has two (the fine octave, pbd_set_fine_octave) -- with p.sbin and
// p.coord those of that bin size; without it, every block of the plan.
template <typename R, int SB, bool RANGE = false>
__global__ __launch_bounds__(256) void k_hog_hist(HogParams p)
{
    __shared__ R bins[18 * 256];
    long long idx0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, end = p.blk_per_frame;
    int lv0 = 0, lv1 = p.nlevels;
    if constexpr (RANGE) { idx0 += p.blk0; end = p.blk1; lv0 = p.lv0; lv1 = p.lv1; }
    const bool active = idx0 < end;
    const long long idx = active ? idx0 : end - 1;
    const int frame = p.frame0 + blockIdx.y;
    const LevelCell c = level_cell<1>(p.lv, find_level_blk<1>(p.lv, lv0, lv1, idx), idx);
    const LevelDesc &d = c.d;
    const int by = c.y, bx = c.x;
    const int sbin = p.sbin;
    const int rows = d.img_rows, cols = d.img_cols;
    const HogPlanes<R> src{static_cast<const R *>(p.gmag) + (size_t)frame * p.pix_per_frame + d.img_off,
                           p.gori + (size_t)frame * p.pix_per_frame + d.img_off, cols};
    const HogCoordT<R> *coord = static_cast<const HogCoordT<R> *>(p.coord);
    R *h = bins + threadIdx.x;
#pragma unroll
    for (int o = 0; o < 18; ++o) h[o * 256] = (R)0;
    HogWindow w = hog_window(sbin, by, bx, d.blk_rows * sbin, d.blk_cols * sbin);
    if (!active) w.yhi = w.ylo;

    if constexpr (SB > 0) hog_walk<R, SB, 256>(coord, w, by, bx, rows, cols, src, h);
    else
    for (int y = w.ylo; y < w.yhi; ++y) {
        const HogCoordT<R> cy = coord[y];
        R wy;
        if (cy.ip == by) wy = cy.v1;            // this block is (iyp, .): weight vy1
        else if (cy.ip + 1 == by) wy = cy.v0;   // this block is (iyp+1, .): weight vy0
        else continue;
        const int ys = y < rows - 2 ? y : rows - 2;
        for (int x = w.xlo; x < w.xhi; ++x) {
            const HogCoordT<R> cx = coord[x];
            R wx;
            if (cx.ip == bx) wx = cx.v1;
            else if (cx.ip + 1 == bx) wx = cx.v0;
            else continue;
            const int xs = x < cols - 2 ? x : cols - 2;
            const size_t g = (size_t)ys * cols + xs;
            // the four scatter lines multiply (vy?*vx?) first, then by v; products commute
            const R contrib = (wy * wx) * src.mag[g];
            R *bin = h + (int)src.ori[g] * 256;
            *bin = *bin + contrib;
        }
    }
    if (!active) return;
    hog_hist_store<R, 256>(h, static_cast<R *>(p.hist) + (size_t)frame * 18 * p.blk_per_frame + idx,
                           static_cast<R *>(p.norm) + (size_t)frame * p.blk_per_frame + idx, p.blk_per_frame);
}

// Fused form of the two passes for the hot case (8-bit BGR frames, T = float, sbin 4 or 8, and 2: the fine octave of an
// sbin-4 model): one workgroup = one tile of
// TBX x TBY blocks.  The gradient magnitude / orientation of the pixels its blocks sample ((TB-1)*SB + 2*SB + 2 per side)
// are computed straight from the level image into LDS, four pixels per lane as in k_hog_grad4, and the block threads
// then walk their windows there: the 5 bytes per pixel of pass 1 never travel to HBM and back (they were 2/3 of the
// two kernels' traffic, each pixel being re-read by four blocks), and the window reads, SB apart between lanes in
// global memory, become LDS reads.  Arithmetic and addition order per bin are those of the two kernels above.
template <int SB, int TBX, int TBY>
__global__ __launch_bounds__(TBX * TBY) void k_hog_tile(HogParams p)
{
    constexpr int NT = TBX * TBY;
    constexpr int LO = (SB + 1) / 2 + 1;                           // pixels sampled left of / above the tile's first block
    constexpr int PWX = SB * (TBX - 1) + (3 * SB + 1) / 2 + 1 + LO, PWY = SB * (TBY - 1) + (3 * SB + 1) / 2 + 1 + LO;
    constexpr int LW = (PWX + 3) & ~3, NQ = LW / 4;
    __shared__ float s_mag[PWY * LW];
    __shared__ uint8_t s_ori[PWY * LW];
    __shared__ float bins[18 * NT];
    const ConvTile tile = p.htiles[blockIdx.x];
    const int frame = p.frame0 + blockIdx.y;
    const LevelDesc d = p.lv[tile.level];
    const int rows = d.img_rows, cols = d.img_cols;
    const int t = threadIdx.x;
    const int ox = SB * tile.x0 - LO, oy = SB * tile.y0 - LO;     // image position of LDS cell (0, 0); ConvTile::{y0, x0} = first block
    const uint8_t *im = p.pyr + ((size_t)frame * p.pix_per_frame + d.img_off) * 3;
    const size_t stride = (size_t)cols * 3;
    const long long npix = (long long)rows * cols;
    for (int q = t; q < PWY * NQ; q += NT) {
        const int py = q / NQ, px = (q - py * NQ) * 4;
        const int y = oy + py, x = ox + px;
        if (y < 1 || y > rows - 2) continue;                       // never sampled (positions are clamped to rows-2 / cols-2)
        const uint8_t *s = im + 3 * x + (size_t)y * stride;
        if (x >= 1 && x + 3 <= cols - 2 && (long long)y * cols + x + 3 < npix) {
            f32x4_u mg;
            uint32_t og;
            hog_grad_quad(s, stride, mg, og);
            *reinterpret_cast<f32x4_u *>(s_mag + py * LW + px) = mg;
            *reinterpret_cast<uint32_t *>(s_ori + py * LW + px) = og;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xi = x + i;
                if (xi < 1 || xi > cols - 2) continue;
                float m; int oo;
                hog_grad_px3<float, uint8_t>(s + 3 * i, stride, m, oo);
                s_mag[py * LW + px + i] = m;
                s_ori[py * LW + px + i] = (uint8_t)oo;
            }
        }
    }
    __syncthreads();
    const int by = tile.y0 + t / TBX, bx = tile.x0 + t % TBX;
    if (by >= d.blk_rows || bx >= d.blk_cols) return;
    float *h = bins + t;
#pragma unroll
    for (int o = 0; o < 18; ++o) h[o * NT] = 0.0f;
    hog_walk<float, SB, NT>(static_cast<const HogCoordT<float> *>(p.coord), hog_window(SB, by, bx, d.blk_rows * SB, d.blk_cols * SB),
                            by, bx, rows, cols, HogLdsTile<LW>{s_mag, s_ori, oy, ox}, h);
    const long long idx = d.blk_off + (long long)by * d.blk_cols + bx;
    hog_hist_store<float, NT>(h, static_cast<float *>(p.hist) + (size_t)frame * 18 * p.blk_per_frame + idx,
                              static_cast<float *>(p.norm) + (size_t)frame * p.blk_per_frame + idx, p.blk_per_frame);
}

// The launches below take one HogGroup each: p.htiles / p.nhtiles are the group's tiles, p.sbin and p.coord its bin size and
// coordinate table, p.blk0 .. p.lv1 its blocks and levels (read by the ranged form only).
bool hog_fused(const HogParams &p, bool f64)
{
    return !f64 && p.depth == kDepth8U && p.cn == 3 && (p.sbin == 2 || p.sbin == 4 || p.sbin == 8);
}

void launch_hog_grad(const HogParams &p, int nframes, bool f64, hipStream_t s)
{
    if (p.pix_per_frame == 0) return;
    if (!f64 && p.depth == kDepth8U && p.cn == 3) {
        dim3 grid4((unsigned)((p.pix_per_frame + 1023) / 1024), nframes);
        PBD_LAUNCH(k_hog_grad4, grid4, dim3(256), 0, s, p);
        return;
    }
    dim3 gridp((unsigned)((p.pix_per_frame + 255) / 256), nframes);
    for_depth(p.depth, [&](auto t) {
        if (f64) PBD_LAUNCH((k_hog_grad<double, decltype(t)>), gridp, dim3(256), 0, s, p);
        else PBD_LAUNCH((k_hog_grad<float, decltype(t)>), gridp, dim3(256), 0, s, p);
    });
}

template <bool RANGE>
static void launch_hog_pass2(const HogParams &p, long long nblk, int nframes, bool f64, hipStream_t s)
{
    if (nblk == 0) return;
    dim3 grid((unsigned)((nblk + 255) / 256), nframes);
    if (f64) PBD_LAUNCH((k_hog_hist<double, 0, RANGE>), grid, dim3(256), 0, s, p);
    else if (p.sbin == 4) PBD_LAUNCH((k_hog_hist<float, 4, RANGE>), grid, dim3(256), 0, s, p);
    else if (p.sbin == 8) PBD_LAUNCH((k_hog_hist<float, 8, RANGE>), grid, dim3(256), 0, s, p);
    else PBD_LAUNCH((k_hog_hist<float, 0, RANGE>), grid, dim3(256), 0, s, p);
}

void launch_hog_hist(const HogParams &p, int nframes, bool f64, bool fused, bool ranged, hipStream_t s)
{
    if (fused) {
        if (p.nhtiles == 0) return;
        dim3 grid((unsigned)p.nhtiles, nframes);
        if (p.sbin == 2) PBD_LAUNCH((k_hog_tile<2, kHogTBX, 16>), grid, dim3(kHogTBX * 16), 0, s, p);
        else if (p.sbin == 4) PBD_LAUNCH((k_hog_tile<4, kHogTBX, 16>), grid, dim3(kHogTBX * 16), 0, s, p);
        else PBD_LAUNCH((k_hog_tile<8, kHogTBX, 8>), grid, dim3(kHogTBX * 8), 0, s, p);
        return;
    }
    if (ranged) launch_hog_pass2<true>(p, p.blk1 - p.blk0, nframes, f64, s);
    else launch_hog_pass2<false>(p, p.blk_per_frame, nframes, f64, s);
}

// ------------------------------------------------------------------------------------------------
// Normalisation and the 32 output channels per interior cell (src/HOGFeatures.cpp:286-340).
// One thread per cell.  The four normalisers are evaluated in double as the reference does.
// PAD: the levels carry a pad (LevelDesc::padx / pady, pbd_set_padding).  The thread of plane cell (y, x) computes interior cell
// (y - pady, x - padx) as above, or writes a pad cell: +0 on channels 0 .. 30 and 1 on channel 31 (featpyramid.m:36-45).  The
// cells leave as in the unpadded form, so a store instruction still covers 1 KB of consecutive addresses.
// ------------------------------------------------------------------------------------------------
template <typename R>
__device__ __forceinline__ R hog_norm(const R *n, int stride)
{
    const R s4 = ((n[0] + n[1]) + n[stride]) + n[stride + 1];
    return (R)(1.0 / sqrt((double)s4 + 0.0001));
}

template <typename R, bool PAD>
__global__ __launch_bounds__(256) void k_hog_feat(HogParams p)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int l = find_level_blk<2>(p.lv, 0, p.nlevels, idx);
    // float: the 32 values of a cell leave through LDS so that a store instruction writes 1 KB of consecutive addresses (a
    // block's 256 cells are consecutive in the feature buffer); written straight from the registers every 16-byte store of a
    // wave touched 64 different 128-byte lines
    constexpr bool VIA_LDS = sizeof(R) == 4;
    constexpr int kPitch = 36;                       // floats per cell in LDS: 16-byte aligned, 4 banks apart
    __shared__ __attribute__((aligned(16))) float tile[VIA_LDS ? 256 * kPitch : 4];
    const bool valid = idx < p.cell_per_frame;
    if (!VIA_LDS && !valid) return;
    const int frame = p.frame0 + blockIdx.y;
    if (valid) {
    const LevelCell c = level_cell<2>(p.lv, l, idx);
    const LevelDesc &d = c.d;
    int y = c.y, x = c.x;
    bool interior = true;
    if constexpr (PAD) {
        y -= d.pady; x -= d.padx;
        interior = y >= 0 && y < d.blk_rows - 2 && x >= 0 && x < d.blk_cols - 2;
    }
    R out[32];
    if (interior) {
    const int bw = d.blk_cols;
    const R *norm = static_cast<const R *>(p.norm) + (size_t)frame * p.blk_per_frame + d.blk_off;
    const R n1 = hog_norm<R>(norm + (size_t)(y + 1) * bw + (x + 1), bw);
    const R n2 = hog_norm<R>(norm + (size_t)y * bw + (x + 1), bw);
    const R n3 = hog_norm<R>(norm + (size_t)(y + 1) * bw + x, bw);
    const R n4 = hog_norm<R>(norm + (size_t)y * bw + x, bw);
    const R *hist = static_cast<const R *>(p.hist) + (size_t)frame * 18 * p.blk_per_frame + d.blk_off + (size_t)(y + 1) * bw + (x + 1);
    R hv[18];
#pragma unroll
    for (int o = 0; o < 18; ++o) hv[o] = hist[(size_t)o * p.blk_per_frame];

    const R lim = (R)0.2;
    R t1 = (R)0, t2 = (R)0, t3 = (R)0, t4 = (R)0;
#pragma unroll
    for (int o = 0; o < 18; ++o) {
        const R val = hv[o];
        R h1 = val * n1; h1 = lim < h1 ? lim : h1;
        R h2 = val * n2; h2 = lim < h2 ? lim : h2;
        R h3 = val * n3; h3 = lim < h3 ? lim : h3;
        R h4 = val * n4; h4 = lim < h4 ? lim : h4;
        out[o] = (R)(0.5 * (double)(((h1 + h2) + h3) + h4));
        t1 += h1; t2 += h2; t3 += h3; t4 += h4;
    }
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const R sum = hv[o] + hv[o + 9];
        R h1 = sum * n1; h1 = lim < h1 ? lim : h1;
        R h2 = sum * n2; h2 = lim < h2 ? lim : h2;
        R h3 = sum * n3; h3 = lim < h3 ? lim : h3;
        R h4 = sum * n4; h4 = lim < h4 ? lim : h4;
        out[18 + o] = (R)(0.5 * (double)(((h1 + h2) + h3) + h4));
    }
    out[27] = (R)(0.2357 * (double)t1);
    out[28] = (R)(0.2357 * (double)t2);
    out[29] = (R)(0.2357 * (double)t3);
    out[30] = (R)(0.2357 * (double)t4);
    out[31] = (R)0;
    } else {
#pragma unroll
        for (int o = 0; o < 31; ++o) out[o] = (R)0;
        out[31] = (R)1;
    }
    typedef R rv4 __attribute__((ext_vector_type(4)));
    if constexpr (VIA_LDS) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<rv4 *>(tile + threadIdx.x * kPitch + 4 * i) = rv4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
    } else {
        R *dst = static_cast<R *>(p.feat) + ((size_t)frame * p.cell_per_frame + idx) * 32;
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<rv4 *>(dst)[i] = rv4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
    }
    }
    if constexpr (VIA_LDS) {
        __syncthreads();
        const long long idx0 = (long long)blockIdx.x * blockDim.x;
        const int nq = (int)min((long long)256, p.cell_per_frame - idx0) * 8;          // 16-byte pieces of this block
        typedef float fv4 __attribute__((ext_vector_type(4)));
        fv4 *dst = reinterpret_cast<fv4 *>(static_cast<float *>(p.feat) + ((size_t)frame * p.cell_per_frame + idx0) * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = (int)threadIdx.x + 256 * i;
            if (j < nq) dst[j] = *reinterpret_cast<const fv4 *>(tile + (j >> 3) * kPitch + (j & 7) * 4);
        }
    }
}

void launch_hog_feat(const HogParams &p, int nframes, bool f64, bool padded, hipStream_t s)
{
    if (p.cell_per_frame == 0) return;
    dim3 grid((unsigned)((p.cell_per_frame + 255) / 256), nframes);
    if (padded) {
        if (f64) PBD_LAUNCH((k_hog_feat<double, true>), grid, dim3(256), 0, s, p);
        else PBD_LAUNCH((k_hog_feat<float, true>), grid, dim3(256), 0, s, p);
        return;
    }
    if (f64) PBD_LAUNCH((k_hog_feat<double, false>), grid, dim3(256), 0, s, p);
    else PBD_LAUNCH((k_hog_feat<float, false>), grid, dim3(256), 0, s, p);
}

}  // namespace pbd
