"""float64 reference and error bounds for the inexact convolution modes (FMA, MFMA, MFMA_F16, MFMA_F64).

Test infrastructure, imported by tests/test_conv_bounds_cpu.py (which pins the yardstick on the CPU) and
tests/test_gpu_conv_modes.py (which holds the kernels to it).

REFERENCE.  ref64() is the "same" correlation of oracle.conv -- out(y, x) = sum_{i,j,c} w[i, j, c] * P[y+i, x+j, c] with
P the feature map bordered by a = k // 2 cells on the top / left (k - 1 - a on the bottom / right), border value 0 on
channels 0..30 and 1 on channel 31 (src/SpatialConvolutionEngine.cpp:147-156) -- summed in float64.  It also returns
M = sum |w| * |P| over the same terms (border cells included), the scale every bound is relative to.

A mode computes the same sum of products of EMULATED operands (mode_ops): MFMA splits every fp32 operand into bf16 terms
x = hi + lo (round to nearest even, hi = bf16(x), lo = bf16(x - hi); x - hi is exact in fp32) and accumulates
hi*hi + hi*lo + lo*hi; MFMA_F16 rounds every operand once to fp16; FMA and MFMA_F64 take the operands as they are.  The
mode's reference is the float64 sum of those products: it differs from the kernel only by the kernel's accumulation.

PER-ELEMENT BOUND.  A sum of n products accumulated in any order in a format of unit roundoff u (an fma or a matrix-core
step rounds at most once per addition) is within gamma_n * sum|products| of the exact sum, gamma_n = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).  The worst case needs every rounding at
its extreme with the same sign; rounding errors behave like independent variables of mean ~0, so the probabilistic
bound sqrt(n) u M with a small multiple holds with overwhelming probability (Higham & Mary, SIAM J. Sci. Comput. 41 (2019)
A2815: |error| <= lambda sqrt(n) u M with probability >= 1 - 2 exp(-lambda^2 / 2) per element; lambda = 8: 1 - 2.5e-14).
So |got - ref| <= 8 sqrt(n) u M (+ extra), n = the products accumulated (3 K for MFMA, K = k * k * 32 otherwise),
u = 2^-24 (fp32 accumulation) or 2^-53 (fp64).  The emulated operands' products are exact in the accumulation format
(bf16 * bf16 and fp16 * fp16 fit fp32's 24 bits), so M of the original operands bounds sum|products| to within 2^-7.
extra: in MFMA_F16 the response itself is stored as fp16, one more rounding of at most half an fp16 ulp of the result
(half_ulp_f16).  Where M == 0 every product is 0 and the response must be exactly 0.
For the fp64 modes the reference is the oracle's own float64 responses (bit-exact with the exact GPU path), which carry
rounding of the same kind: the per-element bound is doubled.

ROOT MEAN SQUARE.  The per-element bound is loose by design (8 sigma, and sqrt(n) where the typical error grows more
slowly), so it only catches gross errors.  A systematic missing term -- a dropped lo product on one tap, one K-step, one
product -- stays below it on most elements, but shifts every element by a relative amount of its own size.  The second
criterion is the RMS of |got - ref| / M over every checked element with M > 0 (in MFMA_F16 the response rounding `extra`
is subtracted first, so the statistic measures the accumulation alone).  A correct fp32 accumulation has a relative error of
order u = 2^-24 per element: with zero-mean weights the partial sums walk like sqrt(k) terms, each rounding contributes
u |partial| / sqrt(3), and the RMS of the total over M is ~u (tests/test_conv_bounds_cpu.py measures 2^-25.5 .. 2^-24.3
for serial fp32 emulations of FMA and MFMA on the GPU tests' inputs).  A missing lo feature term is up to 2^-9 of one of
the K products, so one dropped product of K = 800 moves an element by ~2^-9 / K of M: the CPU test measures an RMS of
2^-18.5 .. 2^-18 for it, one K-step (16 products) 2^-16, one tap (32) 2^-15.5.  The bar sits between: RMS_BAR[fp32] =
2^-20, at least 10x over the correct modes and under every mutant the CPU test emulates.  fp64: the same bar scaled by
2^-29 (the ratio of the two unit roundoffs), 2^-49; correct fp64 accumulations measure 2^-56 .. 2^-55.
"""
from __future__ import annotations

import numpy as np

FLEN = 32
U32 = 2.0 ** -24
U64 = 2.0 ** -53
LAMBDA = 8.0
RMS_BAR = {U32: 2.0 ** -20, U64: 2.0 ** -49}
F16_INF = 65520.0          # |v| >= 65520 rounds to +-inf in fp16 (include/pbd.h)


# ---- operand emulations -------------------------------------------------------------------------------------------------
def bf16(x):
    """fp32 -> bf16 with round to nearest even (as a float32 array); NaN / Inf do not occur in these tests"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split_bf16(x):
    """x = hi + lo (+ the dropped rest): hi = bf16(x), lo = bf16(x - hi); x - hi is exact in fp32"""
    x = np.asarray(x, np.float32)
    hi = bf16(x)
    return hi, bf16(x - hi)


def f16(x):
    """fp32 -> fp16 -> fp32, round to nearest even (subnormals kept)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def f16_response(v):
    """the F16 mode's stored response: fp16 rounding, +-inf at |v| >= 65520 (include/pbd.h)"""
    return f16(v)


def half_ulp_f16(v):
    """half an fp16 ulp at |v| (2^-25 in the subnormal range), the most the response rounding can move v"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.ldexp(1.0, (e - 11).astype(np.int64))


def mode_ops(mode):
    """(feature, weight) operand pairs whose products a mode accumulates; each entry maps an fp32 array to its emulation"""
    if mode in ("fma", "f64", "exact", "identity"):
        return [(lambda x: x, lambda x: x)]
    if mode == "mfma":
        hi = lambda x: split_bf16(x)[0]
        lo = lambda x: split_bf16(x)[1]
        return [(hi, hi), (lo, hi), (hi, lo)]            # feature x weight: hi*hi + hi*lo (feature lo) + lo*hi (weight lo)
    if mode == "f16":
        return [(f16, f16)]
    raise ValueError(mode)


def products(mode, K):
    """n: products accumulated per response element for a filter of K = k*k*32 weights"""
    return 3 * K if mode == "mfma" else K


# ---- the float64 correlation --------------------------------------------------------------------------------------------
def padded(feat, k, dtype=None):
    """(H, W*32) -> (H+k-1, W+k-1, 32) with the convolution's constant border (0, but 1 on channel 31)"""
    feat = np.asarray(feat)
    dtype = dtype or feat.dtype
    H, W = feat.shape[0], feat.shape[1] // FLEN
    a = k // 2
    P = np.zeros((H + k - 1, W + k - 1, FLEN), dtype)
    P[..., FLEN - 1] = 1
    P[a:a + H, a:a + W] = feat.reshape(H, W, FLEN)
    return P


def _corr(P, Wk, H, W):
    """P (H+k-1, W+k-1, 32), Wk (F, k, k, 32), both float64 -> (F, H, W) in float64"""
    F, k = Wk.shape[0], Wk.shape[1]
    out = np.zeros((H, W, F))
    for i in range(k):
        for j in range(k):
            out += P[i:i + H, j:j + W, :] @ Wk[:, i, j, :].T
    return np.moveaxis(out, 2, 0)


def ref64(feat, filters, ksize=None, mode="identity"):
    """feat (H, W*32), filters: a list of (k, k*32) arrays (sizes may differ) -> (ref, M), each (F, H, W) float64.
    ref: the float64 sum of the products of `mode`'s emulated operands (mode_ops); M = sum |w| |f| of the unemulated ones.
    ksize: optional list of the filter sides, checked against the shapes."""
    filters = [np.asarray(f) for f in filters]
    ks = [f.shape[0] for f in filters]
    if ksize is not None:
        assert list(np.broadcast_to(ksize, len(ks))) == ks, (ksize, ks)
    H, W = feat.shape[0], feat.shape[1] // FLEN
    ref = np.zeros((len(filters), H, W))
    M = np.zeros((len(filters), H, W))
    if H * W == 0 or not filters:
        return ref, M
    for k in sorted(set(ks)):
        ids = [i for i, kk in enumerate(ks) if kk == k]
        wk = np.stack([filters[i].reshape(k, k, FLEN) for i in ids])
        P = padded(feat, k)
        for fop, wop in mode_ops(mode):
            ref[ids] += _corr(fop(P).astype(np.float64), wop(wk).astype(np.float64), H, W)
        M[ids] = _corr(np.abs(P).astype(np.float64), np.abs(wk).astype(np.float64), H, W)
    return ref, M


def bound(M, n, u, extra=0.0, both_rounded=False):
    """per-element bound: LAMBDA sqrt(n) u M (+ extra); doubled when the reference is rounded as well (fp64 modes)"""
    b = LAMBDA * np.sqrt(np.asarray(n, np.float64)) * u * M
    return (2.0 * b if both_rounded else b) + extra


# ---- the check ----------------------------------------------------------------------------------------------------------
class Stats:
    """what check() found over one or more planes; `+` merges.  worst: max |got - ref| / bound (<= 1 passes);
    rms: RMS of the relative error over the elements with M > 0; elem_ok: the per-element criterion held everywhere."""

    def __init__(self, u, elem_ok=True, worst=0.0, ss=0.0, count=0, bad=""):
        self.u, self.elem_ok, self.worst, self.ss, self.count, self.bad = u, elem_ok, worst, ss, count, bad

    def __add__(self, o):
        assert o.u == self.u
        return Stats(self.u, self.elem_ok and o.elem_ok, max(self.worst, o.worst), self.ss + o.ss, self.count + o.count,
                     self.bad or o.bad)

    @property
    def rms(self):
        return float(np.sqrt(self.ss / self.count)) if self.count else 0.0

    @property
    def bar(self):
        return RMS_BAR[self.u]

    @property
    def rms_ok(self):
        return self.rms <= self.bar

    @property
    def ok(self):
        return self.elem_ok and self.rms_ok

    def __repr__(self):
        return (f"Stats(elem_ok={self.elem_ok}, worst={self.worst:.3g} of the bound, rms={self.rms:.3g} = 2^{np.log2(self.rms or 1e-300):.2f}, "
                f"rms/bar={self.rms / self.bar:.3g}, n={self.count}{', ' + self.bad if self.bad else ''})")


def check(got, ref, M, n, u, extra=0.0, both_rounded=False, where=""):
    """Both criteria on one array of responses (any shape; n, extra broadcast against it).  Returns Stats; assert_ok()
    or Stats.ok decide.  Non-finite responses fail the element criterion."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    M = np.asarray(M, np.float64)
    err = np.abs(got - ref)
    b = bound(M, n, u, extra, both_rounded)
    b = np.broadcast_to(b, err.shape)
    zero = M == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ok_elem = np.where(zero, got == 0, err <= b)
        ratio = np.where(zero, np.where(got == 0, 0.0, np.inf), err / np.where(b > 0, b, 1.0))
    ok_elem &= np.isfinite(got)
    elem_ok = bool(ok_elem.all())
    bad = ""
    if not elem_ok:
        i = np.unravel_index(int(np.argmin(ok_elem.ravel())), ok_elem.shape) if ok_elem.ndim else ()
        bad = (f"{where} first failure at {tuple(int(v) for v in i)}: got {got[i]!r} ref {ref[i]!r} M {M[i]!r} bound {b[i]!r}; "
               f"{int((~ok_elem).sum())} of {ok_elem.size} fail")
    pos = ~zero
    rel = np.maximum(err[pos] - np.broadcast_to(extra, err.shape)[pos], 0.0) / M[pos]
    rel = np.where(np.isfinite(rel), rel, 1.0)
    worst = float(np.max(np.where(np.isfinite(ratio), ratio, 1e300))) if ratio.size else 0.0
    return Stats(u, elem_ok, worst, float(np.sum(rel * rel)), int(rel.size), bad)


def assert_ok(stats, what=""):
    assert stats.elem_ok, f"{what}: per-element bound fails: {stats}"
    assert stats.rms_ok, f"{what}: RMS {stats.rms:.3g} over the bar {stats.bar:.3g}: {stats}"


def f16_check(got, ref, M, n, where=""):
    """MFMA_F16: the accumulation bound (fp32, n products) plus half an fp16 ulp of the result; responses whose reference
    is past 65520 by more than the bound must be +-inf of the right sign, and none may lie in the ambiguous band"""
    got = np.asarray(got, np.float64)
    acc_b = bound(M, n, U32)
    big = np.abs(ref) - acc_b >= F16_INF
    amb = ~big & (np.abs(ref) + acc_b >= F16_INF - half_ulp_f16(F16_INF))
    assert not amb.any(), f"{where}: a reference within the bound of fp16 overflow; choose other inputs"
    s = check(np.where(big, 0.0, got), np.where(big, 0.0, ref), np.where(big, 0.0, M), n, U32,
              extra=half_ulp_f16(np.abs(ref) + acc_b), where=where)
    inf_ok = bool(np.all(got[big] == np.sign(ref[big]) * np.inf))
    if not inf_ok:
        s.elem_ok, s.bad = False, s.bad or f"{where}: a response past 65520 is not +-inf"
    return s


# ---- inputs shared by the CPU and GPU tests -----------------------------------------------------------------------------
def uniform_features(rng, H, W, scale=0.4, c31=0.0):
    """features in [0, scale) on channels 0..30, channel 31 = c31 (the HOG pyramid writes 0 there)"""
    f = (rng.random((H, W * FLEN), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    if f.size:
        f.reshape(H, W, FLEN)[:, :, FLEN - 1] = c31
    return f


def normal_filters(rng, ks, sigma=0.05):
    """one (k, k*32) filter of sigma * N(0, 1) weights per entry of ks"""
    return [(rng.standard_normal((k, k * FLEN)) * sigma).astype(np.float32) for k in ks]


def zero_mean_filters(rng, ks, sigma=0.05):
    """filters whose weights sum to 0 on every channel, so that responses on a flat feature map cancel"""
    out = []
    for f in normal_filters(rng, ks, sigma):
        k = f.shape[0]
        w = f.reshape(k * k, FLEN).astype(np.float64)
        w -= w.mean(axis=0, keepdims=True)
        out.append(w.astype(np.float32).reshape(k, k * FLEN))
    return out


def model_filters(flat, dtype=np.float32):
    """a FlatModel's filter bank as a list of (k, k*32) arrays of dtype (filters_f32 or filters_f64, as the handle takes it)"""
    src = flat.filters_f32 if np.dtype(dtype) == np.float32 else flat.filters_f64
    out = []
    for f in range(flat.nfilters):
        k, o = int(flat.filter_ksize[f]), int(flat.filter_offset[f])
        out.append(src[o:o + k * k * FLEN].reshape(k, k * FLEN))
    return out
