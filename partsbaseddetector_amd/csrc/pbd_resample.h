// pbd_resample.h (private) -- the per-pixel operations of cv::resize INTER_LINEAR as this library restates it, one definition
// each, for the kernels that resample: the pyramid's resized levels (pbd_kernels_features.hip) and the warped positives
// (pbd_kernels_warp.hip).  The files that include it are compiled with -ffp-contract=off: no multiply-add is fused.
#pragma once

#include "pbd_internal.h"

#include <type_traits>

namespace pbd {

// depth code of an image -> its pixel type, as f(PT{})
template <typename F> void for_depth(int depth, F &&f)
{
    if (depth == kDepth16U) f(uint16_t{});
    else if (depth == kDepth32F) f(float{});
    else if (depth == kDepth64F) f(double{});
    else f(uint8_t{});
}

// The three bytes of a BGR pixel in one (unaligned) 32-bit load: byte loads cost a full memory instruction
// each, and these kernels are bound by the number of them.  The fourth byte belongs to the next pixel (the
// pyramid buffer carries 4 bytes of slack; callers' frames use the byte path for their very last pixel).
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t load_px3(const uint8_t *q) { return *reinterpret_cast<const u32_unaligned *>(q); }
__device__ __forceinline__ uint32_t load_px3_bytes(const uint8_t *q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16); }
__device__ __forceinline__ int px_ch(uint32_t v, int c) { return (int)((v >> (8 * c)) & 0xffu); }

// ------------------------------------------------------------------------------------------------
// cv::resize, INTER_LINEAR, 8-bit (call site src/HOGFeatures.cpp:116).  Coefficient tables are
// built on the host (resize_taps, pbd_handle.h); here: horizontal pass in int, vertical pass
// ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2 >> 2.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int resize_fix(int s00, int s01, int s10, int s11, const ResizeTabX &tx, const ResizeTabY &ty)
{   // one channel from its four taps s<row><column>
    const int r0 = s00 * tx.a0 + s01 * tx.a1;
    const int r1 = s10 * tx.a0 + s11 * tx.a1;
    return (((ty.b0 * (r0 >> 4)) >> 16) + ((ty.b1 * (r1 >> 4)) >> 16) + 2) >> 2;
}

// The other depths (16U, 32F, 64F): cv::resize keeps float coefficients and works in float (double for 64F);
// D = S[sx]*a0 + S[sx+1]*a1 (exactly S[sx] at the last column), dst = cast(R0*b0 + R1*b1), cast = cvRound + clamp for
// 16U (third-party arithmetic restated from OpenCV's generic code path; unpinned, as for 8-bit).
template <typename PT> struct ResizeWork { typedef float type; };
template <> struct ResizeWork<double> { typedef double type; };

template <typename PT, typename WT> __device__ __forceinline__ PT resize_cast(WT v)
{
    if constexpr (std::is_same<PT, uint16_t>::value) {
        const int iv = __float2int_rn(v);
        return (uint16_t)(iv < 0 ? 0 : iv > 65535 ? 65535 : iv);
    } else return v;
}

template <typename PT>
__device__ __forceinline__ PT resize_typed(const PT *S0, const PT *S1, int cn, int c, const ResizeTabXf &tx, const ResizeTabYf &ty)
{
    typedef typename ResizeWork<PT>::type WT;
    WT r0, r1;
    if (tx.last) {
        r0 = (WT)S0[tx.sx * cn + c] * (WT)1; r1 = (WT)S1[tx.sx * cn + c] * (WT)1;
    } else {
        r0 = (WT)S0[tx.sx * cn + c] * (WT)tx.a0 + (WT)S0[(tx.sx + 1) * cn + c] * (WT)tx.a1;
        r1 = (WT)S1[tx.sx * cn + c] * (WT)tx.a0 + (WT)S1[(tx.sx + 1) * cn + c] * (WT)tx.a1;
    }
    return resize_cast<PT, WT>(r0 * (WT)ty.b0 + r1 * (WT)ty.b1);
}

}  // namespace pbd
