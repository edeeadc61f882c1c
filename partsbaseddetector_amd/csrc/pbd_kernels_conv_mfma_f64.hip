// pbd_kernels_conv_mfma_f64.hip -- the filter bank of a T = double handle on the fp64 matrix cores (gfx950).
//
// Opt-in mode PBD_CONV_MFMA_F64.  The same dense contraction as the float matrix-core path (pbd_kernels_conv_mfma.hip),
//
//   out[filter][pixel] = sum_{tap, channel} W[filter][tap][channel] * F[pixel + tap][channel]
//
// but with fp64 operands and fp64 accumulation (v_mfma_f64_16x16x4_f64): no operand is rounded, only the order of the
// sums differs from the reference's, so responses agree with PBD_CONV_EXACT to fp64 rounding (~1e-13 relative), not
// bit for bit.  Every filter size 1..kConvMaxK, one launch per size class, all 32 channels computed (out-of-image cells
// carry the reference's constant border: 0, but 1 on channel 31 -- src/SpatialConvolutionEngine.cpp:147-156).
//
// One MFMA: M = 16 filters (A), N = 16 consecutive pixels of a tile row (B), K = 4 channels.  Fragment layout, checked with
// exact integer data by tools/probes/mfma_f64_layout.hip:
//   A: lane l holds A[l & 15][l >> 4]      B: lane l holds B[l >> 4][l & 15]      (one double per lane)
//   D: four doubles per lane, register r holds D[row = (l >> 4) + 4 r][col = l & 15]
//
// Workgroup = one 32 x 8 tile of the uniform tiling (ConvParams::tiles) of one level / frame x one PASS of mb <= kMfmaMaxMB
// M-tiles (16 filters each), four waves.  Wave w owns tile rows 2w, 2w + 1 = four N-tiles, and all mb M-tiles of the pass:
// mb x 4 accumulators of 16 x 16 (8 VGPRs each), so every weight fragment feeds four MFMAs and every feature fragment mb.
//   Features: the haloed tile sits in LDS in channel blocks of CB = 4 QN channels (16, 8 or 4: the largest whose tile stays
//     within kF64LdsTarget, so two workgroups share a CU -- 5 x 5: 432 cells x 144 B = 62 KB), one record of CB doubles
//     + 16 B of padding per cell.  Lane group g = l >> 4 reads channels g QN .. g QN + QN - 1 of its pixel's cell; the
//     record pitch (144 / 80 / 48 B) makes the 16-byte (8-byte) reads of 16 consecutive cells bank-conflict free.  MFMA q
//     of a tap sums channels {g QN + q : g = 0..3}; the host orders the weights to match.
//   Weights: A-fragments straight from global memory / L2, built on the host in the order a pass reads them
//     ([pass: step][M-tile][q][lane], step = (channel block, tap, q-pair)), one coalesced 512-byte load per fragment.
//   One STEP = one tap x one q-pair (two MFMAs per accumulator when QN >= 2): its fragments are loaded while the MFMAs of
//   the previous step run (two register buffers with static indices).
//   D: pixels on lanes, filters in registers: a store instruction writes four runs of 16 consecutive x.
#include "pbd_internal.h"

#include <algorithm>
#include <type_traits>

namespace pbd {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <int QN> struct F64Blk {
    static constexpr int CB = 4 * QN;                  // channels per staged block
    static constexpr int REC = CB * 8 + 16;            // bytes per cell record in LDS
    static constexpr int QS = QN < 2 ? QN : 2;         // doubles per feature read (one q-pair)
    static constexpr int QP = QN / QS;                 // q-pairs per tap
};

// one pass of MB M-tiles (the passes of a class differ in size by one at most)
template <int QN, int MB>
__device__ __forceinline__ void conv_mfma_f64_pass(const ConvParams &p, const double *__restrict__ wpass, int m0,
                                                   const double *__restrict__ feat, unsigned char *sm, const ConvTile tile,
                                                   const LevelDesc &d, int frame)
{
    using B = F64Blk<QN>;
    constexpr int CB = B::CB, REC = B::REC, QS = B::QS, QP = B::QP, NB = 4;
    typedef typename std::conditional<QS == 2, f64x2, double>::type BT;
    const int H = d.rows, W = d.cols, K = p.ksize, a = K / 2;
    const int PW = kConvTW + K - 1, PH = kConvTH + K - 1, NCELL = PW * PH;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int g = lane >> 4, c16 = lane & 15;

    // stage channel block cb: thread = (cell, pair of channels), UB independent 16-byte loads in flight per batch
    auto stage = [&](int cb) {
        constexpr int NPAIR = CB / 2, UB = 4;
        const int ntask = NCELL * NPAIR;
        for (int base = 0; base < ntask; base += 256 * UB) {
            f64x2 v[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int idx = base + u * 256 + t;
                const int ci = idx / NPAIR, j = idx - ci * NPAIR;
                const int cy = ci / PW, cx = ci - cy * PW;
                const int gy = tile.y0 + cy - a, gx = tile.x0 + cx - a;
                const int c = cb * CB + 2 * j;
                v[u] = f64x2{0.0, c + 1 == 31 ? 1.0 : 0.0};
                if (idx < ntask && gy >= 0 && gy < H && gx >= 0 && gx < W)
                    v[u] = *reinterpret_cast<const f64x2 *>(feat + ((size_t)gy * W + gx) * 32 + c);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int idx = base + u * 256 + t;
                if (idx < ntask) {
                    const int ci = idx / NPAIR, j = idx - ci * NPAIR;
                    *reinterpret_cast<f64x2 *>(sm + (size_t)ci * REC + 16 * j) = v[u];
                }
            }
        }
    };

    // N-tile n of the wave: tile row 2 wv + (n >> 1), columns (n & 1) * 16 .. + 15; byte offsets in the haloed tile
    const int cell0 = ((2 * wv) * PW + c16) * REC + g * QN * 8;
    auto noff = [&](int n) { return ((n >> 1) * PW + (n & 1) * 16) * REC; };
    f64x4 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int NSTEP = K * K * QP;                      // steps per channel block
    BT bq[2][NB];
    double aq[2][MB][QS];
    // fragments of step s of channel block cb into buffer `buf`
    auto load = [&](int buf, int cb, int s) {
        const int tap = s / QP, qp = s - tap * QP;
        const int ti = tap / K, tj = tap - ti * K;
        const unsigned char *bb = sm + cell0 + (ti * PW + tj) * REC + qp * 16;
#pragma unroll
        for (int n = 0; n < NB; ++n) bq[buf][n] = *reinterpret_cast<const BT *>(bb + noff(n));
        const double *ws = wpass + ((size_t)cb * NSTEP + s) * (MB * QS * 64) + lane;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int e = 0; e < QS; ++e) aq[buf][m][e] = ws[(m * QS + e) * 64];
    };
    auto comp = [&](int buf) {
#pragma unroll
        for (int e = 0; e < QS; ++e)
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    double b;
                    if constexpr (QS == 2) b = bq[buf][n][e]; else b = bq[buf][n];
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[buf][m][e], b, acc[m][n], 0, 0, 0);
                }
    };
#pragma unroll 1
    for (int cb = 0; cb < 32 / CB; ++cb) {
        if (cb) __syncthreads();                       // every wave is done with the previous block
        stage(cb);
        __syncthreads();
        load(0, cb, 0);
#pragma unroll 1
        for (int s = 0; s < NSTEP; s += 2) {
            load(1, cb, min(s + 1, NSTEP - 1));        // (the last odd step re-reads step NSTEP - 1: in bounds, unused)
            comp(0);
            load(0, cb, min(s + 2, NSTEP - 1));
            if (s + 1 < NSTEP) comp(1);
        }
    }

    // stores: register r of accumulator (m, n) is filter (m0 + m) * 16 + g + 4 r of pixel c16 of N-tile n
    const size_t HW = (size_t)H * W;
    double *rbase = static_cast<double *>(p.resp) + ((size_t)frame * p.cell_per_frame + d.cell_off) * p.F;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int y = tile.y0 + 2 * wv + (n >> 1), x = tile.x0 + (n & 1) * 16 + c16;
        if (x >= W || y >= H) continue;
        double *rp = rbase + (size_t)y * W + x;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = (m0 + m) * 16 + g + 4 * r;
                if (f < p.nf) rp[(size_t)(p.fmap ? p.fmap[f] : f) * HW] = acc[m][n][r];
            }
    }
}

// grid: (tiles, passes, frames); the mtiles M-tiles of the class are split into `passes` passes of near-equal size
template <int QN>
__global__ __launch_bounds__(256, 2) void k_conv_mfma_f64(ConvParams p, const double *__restrict__ wfrag, int mtiles, int passes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    const ConvTile tile = p.tiles[blockIdx.x];
    const int frame = p.frame0 + blockIdx.z;
    const LevelDesc d = p.lv[tile.level];
    const double *feat = static_cast<const double *>(p.feat) + ((size_t)frame * p.cell_per_frame + d.cell_off) * 32;
    const int m0 = mfma_pass_begin(blockIdx.y, mtiles, passes), mb = mfma_pass_begin(blockIdx.y + 1, mtiles, passes) - m0;
    // a pass's fragments start after those of the M-tiles before it: 8 K^2 fragments of 64 doubles per M-tile
    const double *wpass = wfrag + (size_t)m0 * 8 * p.ksize * p.ksize * 64;
    static_assert(kMfmaMaxMB == 4, "the dispatch below covers pass sizes 1..4");
    switch (mb) {
    case 4: conv_mfma_f64_pass<QN, 4>(p, wpass, m0, feat, smraw, tile, d, frame); break;
    case 3: conv_mfma_f64_pass<QN, 3>(p, wpass, m0, feat, smraw, tile, d, frame); break;
    case 2: conv_mfma_f64_pass<QN, 2>(p, wpass, m0, feat, smraw, tile, d, frame); break;
    default: conv_mfma_f64_pass<QN, 1>(p, wpass, m0, feat, smraw, tile, d, frame); break;
    }
}

size_t conv_mfma_f64_lds(int ksize, int qn)
{
    return (size_t)(kConvTW + ksize - 1) * (kConvTH + ksize - 1) * (4 * qn * 8 + 16);
}

int conv_mfma_f64_qn(int ksize)
{   // the widest channel block whose haloed tile leaves room for two workgroups per CU (4 channels at least)
    int qn = 4;
    while (qn > 1 && conv_mfma_f64_lds(ksize, qn) > kF64LdsTarget) qn /= 2;
    return qn;
}

// the kernel of a channel block: fn(k_conv_mfma_f64<qn>)
template <typename Fn> static void with_variant(int qn, Fn &&fn)
{
    if (qn == 4) fn(k_conv_mfma_f64<4>); else if (qn == 2) fn(k_conv_mfma_f64<2>); else fn(k_conv_mfma_f64<1>);
}

hipError_t conv_mfma_f64_set_lds_limits()
{   // per variant, the largest tile its block size is chosen for: the widest filter at QN = 1, the target otherwise
    hipError_t e = hipSuccess;
    for (int qn = 4; qn >= 1; qn /= 2)
        with_variant(qn, [&](auto k) {
            const size_t cap = qn == 1 ? conv_mfma_f64_lds(kConvMaxK, 1) : kF64LdsTarget;
            if (!e)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
        });
    return e;
}

void launch_conv_mfma_f64(const ConvParams &p, const double *wfrag, int nframes, hipStream_t s)
{
    if (p.ntiles == 0 || p.nf == 0) return;
    const int mtiles = (p.nf + 15) / 16, passes = mfma_passes(mtiles);
    const int qn = conv_mfma_f64_qn(p.ksize);
    with_variant(qn, [&](auto k) {
        PBD_LAUNCH(k, dim3(p.ntiles, passes, nframes), dim3(256), (unsigned)conv_mfma_f64_lds(p.ksize, qn), s, p, wfrag, mtiles,
                   passes);
    });
}

}  // namespace pbd
