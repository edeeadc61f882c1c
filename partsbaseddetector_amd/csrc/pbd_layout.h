// pbd_layout.h (private) -- the weight layouts of the convolution kernels, one definition each, for the host packer
// (upload_filters_t, pbd_capi.hip) and the in-place model update's kernels (pbd_kernels_model.hip) alike.  Every layout is
// stated in gather form: the function takes a DESTINATION index of the packed table and returns the value it holds -- the
// class-local filter, the tap (row-major, i * k + j) and the channel -- or filter -1 for a padding slot, which stays zero.
// A filter block of the model holds its value at tap * 32 + channel.  Plain C++ outside hipcc (tests/test_model_update_cpu.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PBD_HD __host__ __device__
#else
#define PBD_HD
#endif

namespace pbd {

struct WeightSrc { int f, t, c; };   // class-local filter (-1: padding), tap, channel
PBD_HD inline int weight_at(const WeightSrc &s) { return s.t * 32 + s.c; }   // its place in the filter's block

// generic bank (any size, T = double): [channel][tap][Fpad]; KK = k * k taps
PBD_HD inline long long generic_bank_size(int KK, int Fpad) { return 32LL * KK * Fpad; }
PBD_HD inline WeightSrc generic_bank_source(long long i, int KK, int Fpad, int nf)
{
    const int fl = (int)(i % Fpad), t = (int)(i / Fpad % KK), c = (int)(i / ((long long)Fpad * KK));
    return WeightSrc{fl < nf ? fl : -1, t, c};
}

// float 5 x 5 bank: [group of 8 filters][channel][tap][8]
PBD_HD inline WeightSrc group_bank_source(long long i, int KK, int nf)
{
    const int q = (int)(i % 8), t = (int)(i / 8 % KK), c = (int)(i / (8LL * KK) % 32), g = (int)(i / (8LL * KK * 32));
    const int fl = g * 8 + q;
    return WeightSrc{fl < nf ? fl : -1, t, c};
}

// k_conv3's units: unit u (first filter f0, ql filters) holds [channel][tap][ql] at its offset; r = index inside the unit
PBD_HD inline long long unit_size(int KK, int ql) { return 32LL * KK * ql; }
PBD_HD inline WeightSrc unit_source(long long r, int KK, int f0, int ql, int nf)
{
    const int q = (int)(r % ql), t = (int)(r / ql % KK), c = (int)(r / ((long long)ql * KK));
    const int fl = f0 + q;
    return WeightSrc{fl < nf ? fl : -1, t, c};
}

// k_conv3's channel-31 border table: case cs = ((top * 3 + bottom) * 3 + left) * 3 + right rows / columns of the 5 x 5 window
// outside the image; tap (i, j) is outside when
PBD_HD inline bool c31_tap_outside(int cs, int i, int j)
{
    const int right = cs % 3, left = cs / 3 % 3, bot = cs / 9 % 3, top = cs / 27;
    return i < top || i > 4 - bot || j < left || j > 4 - right;
}

// The pass rule of PBD_CONV_MFMA_F64 and PBD_CONV_MFMA_ANY / _F16_ANY: the mtiles M-tiles of a size class run in mfma_passes()
// passes (grid y) of at most kMfmaMaxMB M-tiles and near-equal size; pass ps covers M-tiles [mfma_pass_begin(ps),
// mfma_pass_begin(ps + 1)).  mfma_pass_of: the pass that holds M-tile mi, as its first M-tile m0 and its size mb.
constexpr int kMfmaMaxMB = 4;
struct MfmaPass { int m0, mb; };
PBD_HD inline int mfma_passes(int mtiles) { return (mtiles + kMfmaMaxMB - 1) / kMfmaMaxMB; }
PBD_HD inline int mfma_pass_begin(int pass, int mtiles, int passes) { return pass * mtiles / passes; }
PBD_HD inline MfmaPass mfma_pass_of(int mi, int mtiles, int passes)
{
    int ps = 0;
    while (ps + 1 < passes && mfma_pass_begin(ps + 1, mtiles, passes) <= mi) ++ps;
    const int m0 = mfma_pass_begin(ps, mtiles, passes);
    return MfmaPass{m0, mfma_pass_begin(ps + 1, mtiles, passes) - m0};
}
// (The names the rule had per mode.  Nothing in this tree calls them.  They stay for one commit because the layout tests of the
// commit before this one, tests/test_conv_mfma_any_cpu.py and tests/test_model_update_cpu.py there, compile this header and
// call them, and a commit must still pass its parent's tests; the next change to this header removes them.)
PBD_HD inline int f64_pass_begin(int pass, int mtiles, int passes) { return mfma_pass_begin(pass, mtiles, passes); }
PBD_HD inline int any_passes(int mtiles) { return mfma_passes(mtiles); }

// PBD_CONV_MFMA_F64: a size class of nf filters is mtiles = ceil(nf / 16) M-tiles in `passes` passes (the rule above).
// A-fragments: [pass][channel block][tap][q-pair][M-tile of the pass][q of the
// pair][lane]; lane l of M-tile m holds filter m * 16 + (l & 15), channel cb * CB + (l >> 4) * QN + qp * QS + e, with
// CB = 4 QN channels per block (QN: conv_mfma_f64_qn of the size), QS = min(QN, 2), QP = QN / QS.  8 * KK * 64 values per M-tile.
PBD_HD inline long long f64_frag_size(int KK, int mtiles) { return (long long)mtiles * 8 * KK * 64; }
PBD_HD inline WeightSrc f64_frag_source(long long o, int KK, int QN, int mtiles, int passes, int nf)
{
    const int QS = QN < 2 ? QN : 2, QP = QN / QS, CB = 4 * QN;
    const long long per_tile = 8LL * KK * 64;
    const auto [m0, mb] = mfma_pass_of((int)(o / per_tile), mtiles, passes);
    long long r = o - m0 * per_tile;
    const int l = (int)(r % 64); r /= 64;
    const int e = (int)(r % QS); r /= QS;
    const int m = (int)(r % mb); r /= mb;
    const int qp = (int)(r % QP); r /= QP;
    const int t = (int)(r % KK), cb = (int)(r / KK);
    const int fl = (m0 + m) * 16 + (l & 15);
    return WeightSrc{fl < nf ? fl : -1, t, cb * CB + (l >> 4) * QN + qp * QS + e};
}

// PBD_CONV_MFMA / PBD_CONV_MFMA_F16: 16-bit A-operand records [pass of 160 filters][tap][k-step][M-tile of 32][hi | lo][lane][8];
// lane (r = lane & 31, hh = lane >> 5) of v_mfma_f32_32x32x16 holds filter r of the M-tile, channels kh * 16 + hh * 8 .. + 7.
// NV = 2 values per weight (bf16 hi, lo) or 1 (fp16); *part = 0: hi (or the fp16 value), 1: lo.  f is the filter id.
constexpr int kWrecFilterBlock = 160, kWrecMT = kWrecFilterBlock / 32;
PBD_HD inline long long wrec_size(int KK, int NV, int nfilters)
{
    return (long long)((nfilters + kWrecFilterBlock - 1) / kWrecFilterBlock) * KK * 2 * kWrecMT * NV * 64 * 8;
}
PBD_HD inline WeightSrc wrec_source(long long i, int KK, int NV, int nfilters, int *part)
{
    const int j = (int)(i % 8); i /= 8;
    const int lane = (int)(i % 64); i /= 64;
    *part = (int)(i % NV); i /= NV;
    const int mt = (int)(i % kWrecMT); i /= kWrecMT;
    const int kh = (int)(i % 2); i /= 2;
    const int t = (int)(i % KK), ps = (int)(i / KK);
    const int f = ps * kWrecFilterBlock + mt * 32 + (lane & 31);
    return WeightSrc{f < nfilters ? f : -1, t, kh * 16 + (lane >> 5) * 8 + j};
}

// PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY: the 16-bit A-fragments of ONE size class of nf filters (any side), mtiles =
// ceil(nf / 32) M-tiles in mfma_passes() passes (the rule above).  The kernel stages the features in blocks
// of CB = 32, 16 or 8 channels; one STEP is one 16-deep k-slice of v_mfma_f32_32x32x16: a tap x 16 channels (CB >= 16), or two
// taps x 8 channels (CB = 8; the second tap of the last step is a pad when KK is odd).  Order:
// [pass][channel block][step][M-tile of the pass][hi | lo][lane][8]; lane (r = lane & 31, hh = lane >> 5) holds class-local
// filter (M-tile) * 32 + r and
//   CB = 32: tap step / 2, channels (step & 1) * 16 + hh * 8 .. + 7          (2 KK steps)
//   CB = 16: tap step,     channels cb * 16 + hh * 8 .. + 7                  (KK steps per block)
//   CB =  8: tap 2 step + hh, channels cb * 8 .. + 7                         (ceil(KK / 2) steps per block)
// NV = 2 values per weight (bf16 hi, lo) or 1 (fp16); *part = 0: hi (or the fp16 value), 1: lo.
PBD_HD inline int any_steps(int KK, int CB) { return CB == 32 ? 2 * KK : CB == 16 ? KK : (KK + 1) / 2; }
PBD_HD inline long long any_frag_size(int KK, int CB, int NV, int nf)
{
    return (long long)((nf + 31) / 32) * (32 / CB) * any_steps(KK, CB) * NV * 64 * 8;
}
PBD_HD inline WeightSrc any_frag_source(long long i, int KK, int CB, int NV, int nf, int *part)
{
    const int mtiles = (nf + 31) / 32, steps = any_steps(KK, CB);
    const long long per_tile = (long long)(32 / CB) * steps * NV * 64 * 8;
    const auto [m0, mb] = mfma_pass_of((int)(i / per_tile), mtiles, mfma_passes(mtiles));
    long long r = i - m0 * per_tile;
    const int j = (int)(r % 8); r /= 8;
    const int lane = (int)(r % 64); r /= 64;
    *part = (int)(r % NV); r /= NV;
    const int m = (int)(r % mb); r /= mb;
    const int s = (int)(r % steps), cb = (int)(r / steps);
    const int hh = lane >> 5, fl = (m0 + m) * 32 + (lane & 31);
    int t, c;
    if (CB == 32) { t = s >> 1; c = (s & 1) * 16 + hh * 8 + j; }
    else if (CB == 16) { t = s; c = cb * 16 + hh * 8 + j; }
    else { t = 2 * s + hh; c = cb * 8 + j; }
    return WeightSrc{fl < nf && t < KK ? fl : -1, t < KK ? t : 0, c};
}

// ---- the 16-bit roundings of those records (integer arithmetic: the same bits on the host and on the device) ---------------
PBD_HD inline uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
PBD_HD inline float bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
// bf16, round to nearest even
PBD_HD inline uint16_t f2bf(float f)
{
    uint32_t u = f32_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
PBD_HD inline float bf2f(uint16_t b) { return bits_f32((uint32_t)b << 16); }
// IEEE binary16, round to nearest even (what v_cvt_f16_f32 does)
PBD_HD inline uint16_t host_f2h(float f)
{
    const uint32_t u = f32_bits(f);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t ax = u & 0x7fffffffu;
    if (ax > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // rounds to >= 65520: inf
    if (ax < 0x33000001u) return sign;                                       // below half the smallest subnormal: 0
    const int e = (int)(ax >> 23) - 127;
    const uint32_t m = (ax & 0x7fffffu) | 0x800000u;
    const int shift = e >= -14 ? 13 : 13 + (-14 - e);                        // bits dropped from the 24-bit significand
    const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1);
    uint32_t q = m >> shift;
    if (rest > half || (rest == half && (q & 1u))) ++q;
    const uint32_t bits = e >= -14 ? (((uint32_t)(e + 15) << 10) + (q - 0x400u)) : q;   // carry propagates into the exponent
    return (uint16_t)(sign | bits);
}
// the record value of weight v: part 0 / 1 of the bf16 split x = hi + lo, or the fp16 value
PBD_HD inline uint16_t wrec_value(float v, bool f16, int part)
{
    if (f16) return host_f2h(v);
    const uint16_t hi = f2bf(v);
    return part == 0 ? hi : f2bf(v - bf2f(hi));
}

}  // namespace pbd
