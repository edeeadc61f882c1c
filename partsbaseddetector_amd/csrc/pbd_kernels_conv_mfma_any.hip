// pbd_kernels_conv_mfma_any.hip -- the float matrix-core convolution for every filter size 1..kConvMaxK (gfx950).
//
// Opt-in modes PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY: the arithmetic of PBD_CONV_MFMA / PBD_CONV_MFMA_F16
// (pbd_conv_mfma16.h: bf16 split x = hi + lo with hi*hi + hi*lo + lo*hi, or one fp16 rounding per operand; fp32
// accumulation by v_mfma_f32_32x32x16_{bf16,f16}; the tile stager and the product step are that header's) with the filter
// side a runtime value of the size class, one launch per class, responses to plane fmap[f] of the full bank.  An all-5 x 5
// bank never comes here: it runs k_conv_mfma<5> (launch_conv_stage).
//
//   out[filter][pixel] = sum_{tap, channel} W[filter][tap][channel] * F[pixel + tap][channel]
//
// Workgroup = one 32 x 8 tile of the uniform tiling (ConvParams::tiles) of one level / frame x one PASS of mb <= kMfmaMaxMB
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
#include "pbd_conv_mfma16.h"

#include <type_traits>

namespace pbd {

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
    mfma16_clear(acc);

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
        mfma16_stage_tile<F16, G>(feat, sm, tile.x0, tile.y0, H, W, a, PW, NCELL, cb * CB, REC, LO);
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
                    for (int n = 0; n < NB; ++n) mfma16_products<F16>(acc, n, wq[j], bq[n], bnext + n * kNStep, LO);
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
    const int m0 = mfma_pass_begin(blockIdx.y, mtiles, passes), mb = mfma_pass_begin(blockIdx.y + 1, mtiles, passes) - m0;
    // a pass's fragments start after those of the M-tiles before it
    const u32x4 *wpass = wfrag + (size_t)m0 * (32 / CB) * any_steps(p.ksize * p.ksize, CB) * NV * 64;
    static_assert(kMfmaMaxMB == 4, "the block shapes below cover passes of 1..4 M-tiles");
    if (mb >= 3) conv_mfma_any_pass<CB, F16, 2, 4>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
    else if (mb == 2) conv_mfma_any_pass<CB, F16, 1, 4>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
    else conv_mfma_any_pass<CB, F16, 1, 2>(p, wpass, m0, mb, feat, sm_any, tile, d, frame);
}

// the kernel of a channel block and mode: fn(k_conv_mfma_any<cb, f16>)
template <typename Fn> static void with_variant(int cb, bool f16, Fn &&fn)
{
    if (f16) {
        if (cb == 32) fn(k_conv_mfma_any<32, true>);
        else if (cb == 16) fn(k_conv_mfma_any<16, true>);
        else fn(k_conv_mfma_any<8, true>);
    } else {
        if (cb == 32) fn(k_conv_mfma_any<32, false>);
        else if (cb == 16) fn(k_conv_mfma_any<16, false>);
        else fn(k_conv_mfma_any<8, false>);
    }
}

hipError_t conv_mfma_any_set_lds_limits()
{   // per variant, the largest tile its channel block is chosen for: the widest filter at CB = 8, the target otherwise
    hipError_t e = hipSuccess;
    for (int f16 = 0; f16 < 2; ++f16)
        for (int cb = 32; cb >= 8; cb /= 2)
            with_variant(cb, f16 != 0, [&](auto k) {
                const size_t cap = cb == 8 ? conv_mfma_any_lds(kConvMaxK, 8, f16 != 0) : kAnyLdsTarget;
                if (!e)
                    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
            });
    return e;
}

int conv_mfma_any_occupancy(int ksize, bool f16)
{   // resident workgroups per CU at this filter side (diagnostics)
    int n = -1;
    const int cb = conv_mfma_any_cb(ksize, f16);
    with_variant(cb, f16, [&](auto k) {
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, conv_mfma_any_lds(ksize, cb, f16));
    });
    return n;
}

void launch_conv_mfma_any(const ConvParams &p, const void *wfrag, bool f16, int nframes, hipStream_t s)
{
    if (p.ntiles == 0 || p.nf == 0) return;
    const int mtiles = (p.nf + 31) / 32, passes = mfma_passes(mtiles);
    const int cb = conv_mfma_any_cb(p.ksize, f16);
    with_variant(cb, f16, [&](auto k) {
        PBD_LAUNCH(k, dim3(p.ntiles, passes, nframes), dim3(256), (unsigned)conv_mfma_any_lds(p.ksize, cb, f16), s,
                   p, static_cast<const u32x4 *>(wfrag), mtiles, passes);
    });
}

}  // namespace pbd
