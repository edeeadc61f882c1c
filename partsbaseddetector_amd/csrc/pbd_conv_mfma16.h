// pbd_conv_mfma16.h (private, device) -- what the two 16-bit matrix-core convolution kernels share, each stated once:
// k_conv_mfma (pbd_kernels_conv_mfma.hip, 5 x 5) and k_conv_mfma_any (pbd_kernels_conv_mfma_any.hip, any side).
//
//   out[filter][pixel] = sum_{tap, channel} W[filter][tap][channel] * F[pixel + tap][channel]
//
// bf16 modes: every fp32 operand is split into two bf16 terms, x = hi + lo (hi = bf16(x), lo = bf16(x - hi)), and
// hi*hi + hi*lo + lo*hi is accumulated in fp32 by v_mfma_f32_32x32x16_bf16: 16 significant bits per operand, relative product
// error ~2^-16, three MFMAs per fp32 MAC tile.  fp16 modes: every operand rounded once to fp16, ONE v_mfma_f32_32x32x16_f16.
// What differs between the kernels stays in their files: the wave-to-block assignment, the prefetch depth, the address maps
// of the fragments and the store epilogue.
#pragma once

#include "pbd_internal.h"

namespace pbd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Stages G 8-channel groups, from channel c0 on, of the haloed tile (origin (x0, y0), halo a, PW cells per row, ncell cells) of
// a level (feat: [H][W][32] fp32) into LDS: one record of `pitch` bytes per cell, [hi | lo] bf16 (lo at byte `lo`) or fp16.
// All 256 threads call it; thread = (cell, 8-channel group); the loads of a batch of UB tasks are issued together (one exposed
// memory latency per batch instead of one per task).
template <bool F16, int G>
__device__ __forceinline__ void mfma16_stage_tile(const float *__restrict__ feat, unsigned char *sm, int x0, int y0, int H, int W,
                                                  int a, int PW, int ncell, int c0, int pitch, int lo)
{
    constexpr int NTHR = 256, UB = 4;
    const int t = threadIdx.x, ntask = ncell * G;
    for (int base = 0; base < ntask; base += NTHR * UB) {
        float4 va[UB], vb[UB];
        bool inside[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int idx = base + u * NTHR + t;
            const int ci = idx / G, cg = idx % G;
            const int cy = ci / PW, cx = ci - cy * PW;
            const int gy = y0 + cy - a, gx = x0 + cx - a;
            inside[u] = idx < ntask && gy >= 0 && gy < H && gx >= 0 && gx < W;
            va[u] = vb[u] = float4{0.f, 0.f, 0.f, 0.f};
            if (inside[u]) {
                const float4 *src = reinterpret_cast<const float4 *>(feat + ((size_t)gy * W + gx) * 32 + c0 + cg * 8);
                va[u] = src[0]; vb[u] = src[1];
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int idx = base + u * NTHR + t;
            if (idx >= ntask) continue;
            const int ci = idx / G, cg = idx % G;
            float v[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vb[u].x, vb[u].y, vb[u].z, vb[u].w};
            // constant border: 1 on channel 31 (SpatialConvolutionEngine.cpp:153-156)
            if (!inside[u] && c0 + cg * 8 + 7 == 31) v[7] = 1.0f;
            unsigned char *rec = sm + ci * pitch + cg * 16;
            if constexpr (F16) {
                f16x8 hv;
#pragma unroll
                for (int j = 0; j < 8; ++j) hv[j] = (_Float16)v[j];
                *reinterpret_cast<f16x8 *>(rec) = hv;
            } else {
                bf16x8 hi, lo8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    hi[j] = (__bf16)v[j];
                    lo8[j] = (__bf16)(v[j] - (float)hi[j]);
                }
                *reinterpret_cast<bf16x8 *>(rec) = hi;
                *reinterpret_cast<bf16x8 *>(rec + lo) = lo8;
            }
        }
    }
}

template <int MB, int NB>
__device__ __forceinline__ void mfma16_clear(f32x16 (&acc)[MB][NB])
{
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][n][e] = 0.0f;
}

// One step's products of N-tile n: the wave's MB weight fragments w (hi, lo or the fp16 value) against the N-tile's feature
// fragment b, then the fetch of the N-tile's next fragment from LDS (bnext; the lo half `lo` bytes on): it is needed a whole
// step later.  bf16: for all mi hi*hi, then for all mi hi*lo, then for all mi lo*hi -- this is the accumulation order of the
// responses and must not change.
template <bool F16, int MB, int NB, int NV>
__device__ __forceinline__ void mfma16_products(f32x16 (&acc)[MB][NB], int n, const u32x4 (&w)[MB][NV], u32x4 (&b)[NV],
                                                const unsigned char *bnext, int lo)
{
    static_assert(NV == (F16 ? 1 : 2), "one fp16 value or the bf16 (hi, lo) pair per operand");
    if constexpr (F16) {
        const f16x8 bf = __builtin_bit_cast(f16x8, b[0]);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
            acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w[mi][0]), bf, acc[mi][n], 0, 0, 0);
    } else {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, b[0]), bl = __builtin_bit_cast(bf16x8, b[1]);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
            acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[mi][0]), bh, acc[mi][n], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
            acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[mi][0]), bl, acc[mi][n], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
            acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[mi][1]), bh, acc[mi][n], 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) b[v] = *reinterpret_cast<const u32x4 *>(bnext + v * lo);
}

}  // namespace pbd
