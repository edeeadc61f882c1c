// pbd_kernels_conv_mfma_any.hip -- the float matrix-core convolution for every filter size 1..kConvMaxK (gfx950).
//
// Opt-in modes PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY: the arithmetic of PBD_CONV_MFMA / PBD_CONV_MFMA_F16
// (pbd_kernels_conv_mfma.hip: bf16 split x = hi + lo with hi*hi + hi*lo + lo*hi, or one fp16 rounding per operand; fp32
// accumulation by v_mfma_f32_32x32x16_{bf16,f16}) with the filter side a runtime value of the size class, one launch per class,
// responses to plane fmap[f] of the full bank.  An all-5 x 5 bank never comes here: it runs k_conv_mfma<5> (launch_conv_stage).
//
//   out[filter][pixel] = sum_{tap, channel} W[filter][tap][channel] * F[pixel + tap][channel]
//
// Workgroup = one 32 x 8 tile of the uniform tiling (ConvParams::tiles) of one level / frame x one PASS of mb <= kAnyMaxMB
// M-tiles (32 filters each), four waves.  An N-tile is one tile row (32 consecutive pixels).
//   Features: the haloed tile sits in LDS in channel blocks of CB = 32, 16 or 8 channels (conv_mfma_any_cb: the largest whose
//     tile stays within kAnyLdsTarget, so two workgroups share a CU; 8 for the widest filters, up to 113 KB at 31 x 31), one record
//     [hi CB | lo CB | 16 B pad] (bf16) or [CB halves | 16 B pad] (fp16) per cell, converted once per workgroup and block.
//     Pitches 144 / 80 / 48 B are odd multiples of 16: the 16-byte reads of 32 consecutive cells are bank-conflict free
//     (fp16, CB = 8: 32 B, two-way).
//   One STEP = one 16-deep MFMA k-slice: 16 channels of one tap (CB >= 16; lane half hh supplies channels 8 hh .. 8 hh + 7),
//     or TWO taps x 8 channels (CB = 8; lane half hh supplies tap 2 s + hh).  With K*K odd the last step's second tap is a pad:
//     its weights are zero (any_frag_source) and its feature operand is tap 0's record -- staged, in-tile data, never LDS the
//     workgroup did not write.  Pad filters of the last M-tile have zero weights and are not stored.
//   Weights: A-fragments straight from global memory / L2 in the order a pass reads them (any_frag_source, pbd_layout.h:
//     [pass][channel block][step][M-tile][hi | lo][lane] x 16 bytes), fetched two steps ahead.
//   Waves: mb >= 3: wave (h, u) owns N-tiles 4h .. 4h+3 and M-tiles 2u, 2u+1 (the 2 x 4 block of k_conv_mfma); mb = 2: M-tile u;
//     mb = 1: every wave owns two N-tiles.  The block shape is uniform over the workgroup (all waves meet the same barriers); a
//     wave whose second M-tile does not exist repeats its first and does not store it.
//   D[filter][pixel]: lanes = pixels, registers = filters -> a store instruction writes runs of 32 consecutive x.
#include "pbd_internal.h"

#include <mutex>
#include <type_traits>

namespace pbd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int CB, bool F16, int MB, int NB>
__device__ __forceinline__ void conv_mfma_any_pass(const ConvParams &p, const u32x4 *__restrict__ wpass, int m0, int mb,
                                                   const float *__restrict__ feat, unsigned char *sm, const ConvTile tile,
                                                   const LevelDesc &d, int frame)
{
    constexpr int NV = F16 ? 1 : 2, REC = CB * 2 * NV + 16, LO = CB * 2, G = CB / 8, NBLK = 32 / CB;
    const int H = d.rows, W = d.cols, K = p.ksize, KK = K * K, a = K / 2;
    const int PW = kConvTW + K - 1, PH = kConvTH + K - 1, NCELL = PW * PH;
    const int NSTEP = any_steps(KK, CB);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r = lane & 31, hh = lane >> 5;

    // stage channel block cb: fp32 -> (hi, lo) bf16 or fp16; thread = (cell, 8-channel group), UB loads in flight per batch
    auto stage = [&](int cb) {
        constexpr int UB = 4;
        const int ntask = NCELL * G;
        for (int base = 0; base < ntask; base += 256 * UB) {
            float4 va[UB], vb[UB];
            bool inside[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int idx = base + u * 256 + t;
                const int ci = idx / G, cg = idx % G;
                const int cy = ci / PW, cx = ci - cy * PW;
                const int gy = tile.y0 + cy - a, gx = tile.x0 + cx - a;
                inside[u] = idx < ntask && gy >= 0 && gy < H && gx >= 0 && gx < W;
                va[u] = vb[u] = float4{0.f, 0.f, 0.f, 0.f};
                if (inside[u]) {
                    const float4 *src = reinterpret_cast<const float4 *>(feat + ((size_t)gy * W + gx) * 32 + cb * CB + cg * 8);
                    va[u] = src[0]; vb[u] = src[1];
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int idx = base + u * 256 + t;
                if (idx >= ntask) continue;
                const int ci = idx / G, cg = idx % G;
                float v[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vb[u].x, vb[u].y, vb[u].z, vb[u].w};
                if (!inside[u] && cb * CB + cg * 8 + 7 == 31) v[7] = 1.0f;   // constant border: 1 on channel 31
                unsigned char *rec = sm + (size_t)ci * REC + cg * 16;
                if constexpr (F16) {
                    f16x8 hv;
#pragma unroll
                    for (int j = 0; j < 8; ++j) hv[j] = (_Float16)v[j];
                    *reinterpret_cast<f16x8 *>(rec) = hv;
                } else {
                    bf16x8 hi, lo;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        hi[j] = (__bf16)v[j];
                        lo[j] = (__bf16)(v[j] - (float)hi[j]);
                    }
                    *reinterpret_cast<bf16x8 *>(rec) = hi;
                    *reinterpret_cast<bf16x8 *>(rec + LO) = lo;
                }
            }
        }
    };

    // the wave's block: N-tiles n0 .. n0 + NB - 1 (tile rows), M-tiles ml[0 .. MB) of the pass (a missing one repeats the first)
    int n0, mfirst;
    if (mb == 1) { n0 = NB * wv; mfirst = 0; }
    else { n0 = NB * (wv >> 1); mfirst = (wv & 1) * MB; }
    int ml[MB];
    bool mok[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) { mok[mi] = mfirst + mi < mb; ml[mi] = mok[mi] ? mfirst + mi : mfirst; }
    const int kNStep = PW * REC;
    const int celln = (n0 * PW + r) * REC;

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][n][e] = 0.0f;

    // byte address of the lane's feature fragment of step s, N-tile 0 of the block
    auto b_addr = [&](int s) {
        int tap, off;
        if constexpr (CB == 32) { tap = s >> 1; off = (s & 1) * 32 + hh * 16; }
        else if constexpr (CB == 16) { tap = s; off = hh * 16; }
        else { tap = 2 * s + hh; if (tap >= KK) tap = 0; off = 0; }   // (pad tap: zero weights against a staged record)
        const int ti = tap / K, tj = tap - ti * K;
        return sm + celln + (ti * PW + tj) * REC + off;
    };
    // fragment (step s, M-tile m of the pass, part v) of channel block cb
    auto a_addr = [&](int cb, int s) { return wpass + ((size_t)cb * NSTEP + s) * mb * NV * 64 + lane; };

    constexpr int PF = 2;
    u32x4 wq[PF][MB][NV], bq[NB][NV];
    auto load_a = [&](int j, int cb, int s) {
        const u32x4 *ws = a_addr(cb, s);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int v = 0; v < NV; ++v) wq[j][mi][v] = ws[(ml[mi] * NV + v) * 64];
    };
    auto load_b = [&](int s) {
        const unsigned char *bb = b_addr(s);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            bq[n][0] = *reinterpret_cast<const u32x4 *>(bb + n * kNStep);
            if constexpr (!F16) bq[n][1] = *reinterpret_cast<const u32x4 *>(bb + n * kNStep + LO);
        }
    };
    // (every wave owns at least its first M-tile: mfirst < mb in all three block shapes, so all waves run the step loop)

#pragma unroll 1
    for (int cb = 0; cb < NBLK; ++cb) {
        if (cb) __syncthreads();                       // every wave is done with the previous block
        stage(cb);
        __syncthreads();
        load_a(0, cb, 0);
        load_a(1, cb, min(1, NSTEP - 1));
        load_b(0);
#pragma unroll 1
        for (int s0 = 0; s0 < NSTEP; s0 += PF) {
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int s = s0 + j;
                if (s < NSTEP) {                       // (uniform; NSTEP may be odd)
                    const unsigned char *bnext = b_addr(min(s + 1, NSTEP - 1));
#pragma unroll
                    for (int n = 0; n < NB; ++n) {
                        if constexpr (F16) {
                            const f16x8 bf = __builtin_bit_cast(f16x8, bq[n][0]);
#pragma unroll
                            for (int mi = 0; mi < MB; ++mi)
                                acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wq[j][mi][0]), bf, acc[mi][n], 0, 0, 0);
                            bq[n][0] = *reinterpret_cast<const u32x4 *>(bnext + n * kNStep);
                        } else {
                            const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[n][0]), bl = __builtin_bit_cast(bf16x8, bq[n][1]);
#pragma unroll
                            for (int mi = 0; mi < MB; ++mi)
                                acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wq[j][mi][0]), bh, acc[mi][n], 0, 0, 0);
#pragma unroll
                            for (int mi = 0; mi < MB; ++mi)
                                acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wq[j][mi][0]), bl, acc[mi][n], 0, 0, 0);
#pragma unroll
                            for (int mi = 0; mi < MB; ++mi)
                                acc[mi][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wq[j][mi][1]), bh, acc[mi][n], 0, 0, 0);
                            bq[n][0] = *reinterpret_cast<const u32x4 *>(bnext + n * kNStep);
                            bq[n][1] = *reinterpret_cast<const u32x4 *>(bnext + n * kNStep + LO);
                        }
                    }
                    load_a(j, cb, min(s + PF, NSTEP - 1));
                }
            }
        }
    }
    // D layout (32x32): column = lane & 31 (pixel), row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) (filter of the M-tile)
    using RT = typename std::conditional<F16, _Float16, float>::type;
    const size_t HW = (size_t)H * W;
    RT *rbase = reinterpret_cast<RT *>(p.resp) + ((size_t)frame * p.cell_per_frame + d.cell_off) * p.F;
    const int x = tile.x0 + r;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        if (!mok[mi]) continue;
        const int f0 = (m0 + ml[mi]) * 32 + 4 * hh;
        long long plane[16];                           // element offset of the lane's 16 response planes, -1: a pad filter
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int f = f0 + (e & 3) + 8 * (e >> 2);
            plane[e] = f < p.nf ? (long long)(p.fmap ? p.fmap[f] : f) * (long long)HW : -1;
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int y = tile.y0 + n0 + n;
            if (x >= W || y >= H) continue;
            RT *rp = rbase + (size_t)y * W + x;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (plane[e] >= 0) rp[plane[e]] = (RT)acc[mi][n][e];
        }
    }
}

// grid: (tiles, passes, frames); the mtiles M-tiles of the class are split into `passes` passes of near-equal size
template <int CB, bool F16>
__global__ __launch_bounds__(256, 2) void k_conv_mfma_any(ConvParams p, const u32x4 *__restrict__ wfrag, int mtiles, int passes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_any[];
    constexpr int NV = F16 ? 1 : 2;
    const ConvTile tile = p.tiles[blockIdx.x];
    const int frame = p.frame0 + blockIdx.z;
    const LevelDesc d = p.lv[tile.level];
    const float *feat = static_cast<const float *>(p.feat) + ((size_t)frame * p.cell_per_frame + d.cell_off) * 32;
    const int m0 = f64_pass_begin(blockIdx.y, mtiles, passes), mb = f64_pass_begin(blockIdx.y + 1, mtiles, passes) - m0;
    // a pass's fragments start after those of the M-tiles before it
    const u32x4 *wpass = wfrag + (size_t)m0 * (32 / CB) * any_steps(p.ksize * p.ksize, CB) * NV * 64;
    static_assert(kAnyMaxMB == 4, "the block shapes below cover passes of 1..4 M-tiles");
    if (mb >= 3) conv_mfma_any_pass<CB, F16, 2, 4>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
    else if (mb == 2) conv_mfma_any_pass<CB, F16, 1, 4>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
    else conv_mfma_any_pass<CB, F16, 1, 2>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
}

template <int CB, bool F16> static hipError_t set_lds_limit()
{   // the largest tile this channel block is chosen for: the widest filter at CB = 8, the target otherwise
    const size_t cap = CB == 8 ? conv_mfma_any_lds(kConvMaxK, 8, F16) : kAnyLdsTarget;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_conv_mfma_any<CB, F16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
}

// Raises the dynamic LDS limit of every variant on the CURRENT device: once per device and process, never per launch (handles
// launch concurrently), and before any launch -- upload_filters_t calls it and reports a failure as its own.
hipError_t conv_mfma_any_prepare()
{
    static std::once_flag once[kAnyMaxDevices];
    static hipError_t result[kAnyMaxDevices];
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= kAnyMaxDevices) return hipErrorInvalidDevice;   // (more devices than the flag table holds)
    std::call_once(once[dev], [dev] {
        hipError_t e = set_lds_limit<32, false>();
        if (!e) e = set_lds_limit<16, false>();
        if (!e) e = set_lds_limit<8, false>();
        if (!e) e = set_lds_limit<32, true>();
        if (!e) e = set_lds_limit<16, true>();
        if (!e) e = set_lds_limit<8, true>();
        result[dev] = e;
    });
    return result[dev];
}

template <int CB, bool F16>
static void launch_any(const ConvParams &p, const void *wfrag, int mtiles, int passes, int nframes, hipStream_t s)
{
    PBD_LAUNCH((k_conv_mfma_any<CB, F16>), dim3(p.ntiles, passes, nframes), dim3(256), (unsigned)conv_mfma_any_lds(p.ksize, CB, F16), s,
               p, static_cast<const u32x4 *>(wfrag), mtiles, passes);
}

int conv_mfma_any_occupancy(int ksize, bool f16)
{   // resident workgroups per CU at this filter side (diagnostics)
    int n = -1;
    const int cb = conv_mfma_any_cb(ksize, f16);
    const size_t lds = conv_mfma_any_lds(ksize, cb, f16);
#define PBD_ANY_OCC(CB, F) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_conv_mfma_any<CB, F>, 256, lds)
    if (f16) { if (cb == 32) PBD_ANY_OCC(32, true); else if (cb == 16) PBD_ANY_OCC(16, true); else PBD_ANY_OCC(8, true); }
    else { if (cb == 32) PBD_ANY_OCC(32, false); else if (cb == 16) PBD_ANY_OCC(16, false); else PBD_ANY_OCC(8, false); }
#undef PBD_ANY_OCC
    return n;
}

void launch_conv_mfma_any(const ConvParams &p, const void *wfrag, bool f16, int nframes, hipStream_t s)
{
    if (p.ntiles == 0 || p.nf == 0) return;
    const int mtiles = (p.nf + 31) / 32, passes = any_passes(mtiles);
    const int cb = conv_mfma_any_cb(p.ksize, f16);
    if (f16) {
        if (cb == 32) launch_any<32, true>(p, wfrag, mtiles, passes, nframes, s);
        else if (cb == 16) launch_any<16, true>(p, wfrag, mtiles, passes, nframes, s);
        else launch_any<8, true>(p, wfrag, mtiles, passes, nframes, s);
    } else {
        if (cb == 32) launch_any<32, false>(p, wfrag, mtiles, passes, nframes, s);
        else if (cb == 16) launch_any<16, false>(p, wfrag, mtiles, passes, nframes, s);
        else launch_any<8, false>(p, wfrag, mtiles, passes, nframes, s);
    }
}

}  // namespace pbd
