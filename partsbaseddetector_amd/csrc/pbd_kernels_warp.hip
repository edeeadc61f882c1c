// pbd_kernels_warp.hip -- warped positives (pbd_warp_positives*): poswarp of the reference's Matlab training code
// (matlab/learning/train.m:131-162, warppos.m, subarray.m, qp_poswrite).  include/pbd.h states the contract, DESIGN.md
// section 6k the design.  Compiled with -ffp-contract=off, as every file that resamples.
//
// Every kept box is one level of a plan of P x P level images, P = (k + 2) * sbin (pbd_capi.hip: warp_plan):
//   k_warp       one thread per destination pixel of every kept box: the four taps of cv::resize INTER_LINEAR over the box's
//                padded window, each tap clamped into the frame on the host (subarray's edge replication: no crop is ever
//                materialised), through resize_fix (8-bit) / resize_typed (16U, 32F, 64F), the operations of the pyramid's
//                resized levels (pbd_resample.h)
//   (the HOG launches of the detect path run over the patches unchanged)
//   k_warp_emit  one workgroup per box: header, payload record and, for a kept box, the bias value and the k x k x flen features
//                as 16-byte chunks (a source chunk is 16-byte aligned; the destination follows one bias value, so it is
//                element aligned, as in k_ex_gather)
// No atomics, and no kernel reads what another workgroup of the same launch writes.
#include "pbd_internal.h"
#include "pbd_resample.h"

namespace pbd {
namespace {

constexpr int kWarpThreads = 256;

template <typename PT>
__global__ __launch_bounds__(kWarpThreads) void k_warp(WarpParams p)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int PP = p.P * p.P;
    if (idx >= (long long)p.nkept * PP) return;
    const int j = (int)(idx / PP), local = (int)(idx - (long long)j * PP);
    const int y = local / p.P, x = local - y * p.P;
    const FrameDesc fr = p.fd[p.box_frame[j]];
    const WarpTap tx2 = p.tapx[(size_t)j * p.P + x];
    const int cn = p.cn;
    PT *dst = reinterpret_cast<PT *>(p.pyr) + (size_t)idx * cn;
    if constexpr (std::is_same<PT, uint8_t>::value) {
        const ResizeTabX tx = static_cast<const ResizeTabX *>(p.cx)[(size_t)j * p.P + x];
        const ResizeTabY ty = static_cast<const ResizeTabY *>(p.cy)[(size_t)j * p.P + y];
        const uint8_t *S0 = fr.data + (size_t)ty.y0 * fr.pitch, *S1 = fr.data + (size_t)ty.y1 * fr.pitch;
        if (cn == 3) {
            // packed loads wherever the pixel's fourth byte lies inside the frame's memory: everywhere but its very last pixel
            auto ld = [&](const uint8_t *row, int yy, int xx) {
                return (yy == fr.rows - 1 && xx == fr.cols - 1) ? load_px3_bytes(row + xx * 3) : load_px3(row + xx * 3);
            };
            const uint32_t p00 = ld(S0, ty.y0, tx2.i0), p01 = ld(S0, ty.y0, tx2.i1), p10 = ld(S1, ty.y1, tx2.i0), p11 = ld(S1, ty.y1, tx2.i1);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                dst[c] = (uint8_t)resize_fix(px_ch(p00, c), px_ch(p01, c), px_ch(p10, c), px_ch(p11, c), tx, ty);
            return;
        }
        for (int c = 0; c < cn; ++c)
            dst[c] = (uint8_t)resize_fix(S0[tx2.i0 * cn + c], S0[tx2.i1 * cn + c], S1[tx2.i0 * cn + c], S1[tx2.i1 * cn + c], tx, ty);
    } else {
        ResizeTabXf tx = static_cast<const ResizeTabXf *>(p.cx)[(size_t)j * p.P + x];
        const ResizeTabYf ty = static_cast<const ResizeTabYf *>(p.cy)[(size_t)j * p.P + y];
        const PT *S0 = reinterpret_cast<const PT *>(fr.data + (size_t)ty.y0 * fr.pitch);
        const PT *S1 = reinterpret_cast<const PT *>(fr.data + (size_t)ty.y1 * fr.pitch);
        tx.sx = 0;   // resize_typed reads its taps at sx and sx + 1 of the rows it is given: the two gathered taps of each row
        for (int c = 0; c < cn; ++c) {
            const PT r0[2] = {S0[tx2.i0 * cn + c], S0[tx2.i1 * cn + c]};
            const PT r1[2] = {S1[tx2.i0 * cn + c], S1[tx2.i1 * cn + c]};
            dst[c] = resize_typed<PT>(r0, r1, 1, 0, tx, ty);
        }
    }
}

template <typename R>
__global__ __launch_bounds__(kWarpThreads) void k_warp_emit(WarpParams p)
{
    constexpr int V = 16 / sizeof(R);
    typedef R vload __attribute__((ext_vector_type(V)));
    typedef R vstore __attribute__((ext_vector_type(V), aligned(sizeof(R))));
    const int i = blockIdx.x, t = threadIdx.x;
    const int j = p.slot[i];
    const int nb0 = p.bias >= 0 ? 1 : 0;
    int32_t *hdr = p.hdr + (size_t)i * p.hdr_words;
    for (int w = t; w < p.hdr_words; w += kWarpThreads) {
        int v = 0;
        if (w == 0) v = i;
        else if (w == 2) v = j < 0 ? -1 : nb0 + 1;
        else if (j >= 0) {
            if (w == 3) v = nb0 + p.filter_len;
            else if (nb0 && w == 4) v = p.bias;
            else if (nb0 && w == 5) v = 1;
            else if (w == 4 + 2 * nb0) v = p.filter_off;
            else if (w == 5 + 2 * nb0) v = p.filter_len;
        }
        hdr[w] = v;
    }
    if (p.payload) {
        if (i == 0 && t == 0) p.payload[0] = p.nboxes;
        int32_t *rec = p.payload + 1 + (size_t)i * p.rec_stride;
        for (int w = t; w < p.rec_stride; w += kWarpThreads) rec[w] = w == 0 ? p.id_offset + i : 0;
    }
    if (j < 0) return;
    R *dst = static_cast<R *>(p.values) + (size_t)i * p.vstride;
    if (nb0 && t == 0) dst[0] = (R)1;
    const R *src = static_cast<const R *>(p.feat) + (size_t)j * p.filter_len;
    for (int q = t; q < p.filter_len / V; q += kWarpThreads)
        *reinterpret_cast<vstore *>(dst + nb0 + (size_t)q * V) = *reinterpret_cast<const vload *>(src + (size_t)q * V);
}

}  // namespace

void launch_warp(const WarpParams &p, hipStream_t s)
{
    const long long npix = (long long)p.nkept * p.P * p.P;
    if (npix == 0) return;
    dim3 grid((unsigned)((npix + kWarpThreads - 1) / kWarpThreads));
    for_depth(p.depth, [&](auto t) { PBD_LAUNCH(k_warp<decltype(t)>, grid, dim3(kWarpThreads), 0, s, p); });
}

void launch_warp_emit(const WarpParams &p, bool f64, hipStream_t s)
{
    if (p.nboxes == 0) return;
    dim3 grid((unsigned)p.nboxes);
    if (f64) PBD_LAUNCH(k_warp_emit<double>, grid, dim3(kWarpThreads), 0, s, p);
    else PBD_LAUNCH(k_warp_emit<float>, grid, dim3(kWarpThreads), 0, s, p);
}

}  // namespace pbd
