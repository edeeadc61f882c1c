"""Inputs shared by the CPU and GPU tests of PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY (tests/test_conv_mfma_any_cpu.py,
tests/test_gpu_conv_mfma_any.py): the one-hot banks, their features, and their reference.

ONE-HOT BANK of side k: k*k filters, filter t all zero except tap t at channel (7 t + 3) mod 32, value +-(1 + 2^-9).  Features
0.25 (1 + 2^-9) 2^e, e per cell from -3 .. 3, channel 31 zero inside the map.  Both operands split into bf16 terms as
hi = 2^m, lo = 2^(m - 9), so hi*hi + hi*lo + lo*hi = 2^(m + m') (1 + 2^-8) is one fp32 number and the only non-zero product of
its response: the bf16 mode must return it exactly, whatever the order of accumulation; the dropped lo*lo term (2^-18 relative)
is what PBD_CONV_FMA adds.  In fp16 both operands are exact, so the response is f16(w * f).

onehot_ref() is conv_reference.ref64() restricted to the products that are not identically zero: the same padded map
(conv_reference.padded), the same operand emulations (conv_reference.mode_ops), summed in float64.  ref64 itself costs
k^4 matrix products on these banks; the CPU test checks that the two agree on whole small banks and on a stride of filters
of the large ones."""
import numpy as np

import conv_reference as R

FLEN = R.FLEN
W_ONE = np.float32(1.0 + 2.0 ** -9)
# sides around every staging change of the host rule (staging_cb below), the smallest and the largest
SIDES_BF16 = [1, 2, 3, 4, 6, 7, 8, 12, 15, 16, 18, 19, 31]
SIDES_F16 = [1, 2, 3, 4, 6, 7, 12, 15, 16, 18, 19, 24, 25, 31]
ONEHOT_LEVELS = [(9, 37), (2, 2), (40, 70)]
TILE_W, TILE_H, LDS_TARGET = 32, 8, 80 * 1024


def staging_cb(k, f16):
    """the channel block of a filter side, as conv_mfma_any_cb (pbd_internal.h) states it: the largest of 32 / 16 / 8 whose
    haloed 32 x 8 tile of [hi | lo | 16 B] (or [fp16 | 16 B]) records fits 80 KB"""
    cb = 32
    while cb > 8 and (TILE_W + k - 1) * (TILE_H + k - 1) * (cb * (2 if f16 else 4) + 16) > LDS_TARGET:
        cb //= 2
    return cb


def onehot_bank(k):
    """(filters, (tap, channel, value) per filter)"""
    filters, where = [], []
    for t in range(k * k):
        c = (7 * t + 3) % FLEN
        v = W_ONE if t % 3 else -W_ONE
        w = np.zeros((k, k * FLEN), np.float32)
        w[t // k, (t % k) * FLEN + c] = v
        filters.append(w)
        where.append((t, c, v))
    return filters, where


def onehot_features(seed, dims):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in dims:
        e = rng.integers(-3, 4, size=(h, w, FLEN))
        f = (np.float32(0.25) * W_ONE * np.ldexp(np.float32(1.0), e)).astype(np.float32)
        f[:, :, FLEN - 1] = 0
        out.append(f.reshape(h, w * FLEN))
    return out


def onehot_ref(feat, k, mode, drop=None, filters=None):
    """(ref, M) of the one-hot bank of side k on one level, float64, (len(filters), H, W); drop = 1 or 2 leaves out that
    operand pair of mode_ops("mfma") (a lo term): the mutants of the CPU test.  filters: indices (default: all k*k)"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    _, where = onehot_bank(k)
    ids = range(k * k) if filters is None else filters
    P = R.padded(feat, k)
    ops = [op for i, op in enumerate(R.mode_ops(mode)) if i != drop]
    Pe = [fop(P).astype(np.float64) for fop, _ in ops]
    ref = np.zeros((len(ids), H, W))
    M = np.zeros((len(ids), H, W))
    for o, f in enumerate(ids):
        t, c, v = where[f]
        i, j = t // k, t % k
        for (fop, wop), pe in zip(ops, Pe):
            ref[o] += pe[i:i + H, j:j + W, c] * np.float64(wop(np.float32(v)))
        M[o] = np.abs(P[i:i + H, j:j + W, c]).astype(np.float64) * abs(np.float64(v))
    return ref, M


def onehot_differs(feat, k):
    """where the full fp32 product (what the vector modes return: lo*lo included) is another fp32 number than the bf16 mode's"""
    full, _ = onehot_ref(feat, k, "identity")
    ref, _ = onehot_ref(feat, k, "mfma")
    return full.astype(np.float32) != ref.astype(np.float32)
