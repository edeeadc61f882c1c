"""Pins the yardstick of tests/test_gpu_conv_modes.py on the CPU (tests/conv_reference.py):

* ref64 is the oracle's correlation (oracle.conv / oracle.responses) to within the bound, in f32 and f64, for every filter
  size the GPU tests use, 1 x 1 maps, maps smaller than the filter, empty maps and a non-zero channel 31;
* ACCEPTANCE: an fp32 / fp64 emulation of each correct mode, accumulating in a different order from the reference, passes
  both criteria on the GPU tests' inputs, with an RMS at least 10x under its bar;
* REJECTION: each emulated mutant -- a dropped split product, a dropped lo term on one tap / one K-step / one product,
  hi-only bf16, bf16 where fp16 belongs, one tap's partial sum rounded through a narrower format, fp64 weights rounded to
  fp32 -- fails at least one criterion.  One parametrized case per mutant, so a mutant that slips through is named."""
import numpy as np
import pytest

import conv_reference as R
from partsbaseddetector_amd import model as MD
from partsbaseddetector_amd import synth

FLEN = R.FLEN


# ---- inputs: what test_gpu_conv_modes.py feeds the kernels, at CPU-friendly sizes -----------------------------------------
@pytest.fixture(scope="module")
def hog_level(oracle):
    """a real HOG level (mostly small, many exact zeros, channel 31 = 0)"""
    flat = MD.synthetic_person_model().flatten()
    feats, _ = oracle.features_pyramid(flat, synth.synthetic_frame(21, 96, 128, 3))
    return np.ascontiguousarray(feats[2])


def _inputs(kind, hog_level):
    rng = np.random.default_rng(1234)
    if kind == "hog":
        return hog_level[:14, :17 * FLEN].copy(), R.normal_filters(rng, [5] * 6)
    if kind == "uniform":
        return R.uniform_features(rng, 13, 15), R.normal_filters(rng, [5] * 6)
    if kind == "zero_mean":
        return R.uniform_features(rng, 13, 15), R.zero_mean_filters(rng, [5] * 6)
    raise ValueError(kind)


KINDS = ["hog", "uniform", "zero_mean"]


def _K(w):
    return w.shape[0] * w.shape[0] * FLEN


def _nvec(filters, mode):
    return np.array([R.products(mode, _K(w)) for w in filters], np.float64)[:, None, None]


# ---- emulations: serial accumulation over (tap, channel), vectorised over (filter, y, x) ----------------------------------
def _terms(feat, filters):
    """(P window (H, W, 32) of tap t, weights (F, 32) of tap t) in raster tap order; 5 x 5 banks only"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    k = filters[0].shape[0]
    assert all(w.shape[0] == k for w in filters)
    P = R.padded(feat, k)
    wk = np.stack([w.reshape(k * k, FLEN) for w in filters])
    for t in range(k * k):
        i, j = divmod(t, k)
        yield t, P[i:i + H, j:j + W, :], wk[:, t, :]


def emu_fma32(feat, filters, tap_f16=None):
    """serial fused accumulation in fp32: one accumulator per element, s = fma(w, f, s) over taps x channels.
    tap_f16: the mutant whose tap `tap_f16` is summed on its own, rounded through fp16 and then added"""
    acc = np.zeros((len(filters),) + feat.shape[:1] + (feat.shape[1] // FLEN,), np.float32)
    for t, win, w in _terms(feat, filters):
        part = np.zeros_like(acc) if t == tap_f16 else acc
        for c in range(FLEN):
            prod = w[:, c, None, None].astype(np.float64) * win[None, :, :, c].astype(np.float64)
            part = (prod + part).astype(np.float32)                  # exact product, one rounding (to within double rounding)
        if t == tap_f16:
            acc = (acc + R.f16(part)).astype(np.float32)
        else:
            acc = part
    return acc


def emu_split32(feat, filters, terms=("hh", "hl", "lh"), drop_hl=lambda t, c: False):
    """the three bf16 split products accumulated serially in fp32 (each product exact in fp32); `terms` and drop_hl(tap,
    channel) make the mutants (hl = feature lo times weight hi)"""
    wsplit = [R.split_bf16(w) for w in filters]
    whi = [a for a, _ in wsplit]
    wlo = [b for _, b in wsplit]
    acc = np.zeros((len(filters), feat.shape[0], feat.shape[1] // FLEN), np.float32)
    for (t, win, wh), (_, _, wl) in zip(_terms(feat, whi), _terms(feat, wlo)):
        fh, fl = R.split_bf16(win)
        for c in range(FLEN):
            for name, fo, wo in (("hh", fh, wh), ("hl", fl, wh), ("lh", fh, wl)):
                if name not in terms or (name == "hl" and drop_hl(t, c)):
                    continue
                acc = (acc + wo[:, c, None, None] * fo[None, :, :, c]).astype(np.float32)
    return acc


def emu_f16(feat, filters, rnd=R.f16):
    """fp16 operands (or the mutant's rounding `rnd`), products exact, serial fp32 accumulation, fp16 response"""
    acc = np.zeros((len(filters), feat.shape[0], feat.shape[1] // FLEN), np.float32)
    for t, win, w in _terms(feat, [rnd(w) for w in filters]):
        fw = rnd(win)
        for c in range(FLEN):
            acc = (acc + w[:, c, None, None] * fw[None, :, :, c]).astype(np.float32)
    return R.f16_response(acc)


def emu_f64(feat, filters, tap_f32=None, w_f32=False):
    """serial fp64 accumulation in tap-major order (the oracle sums channel-major); mutants: tap `tap_f32`'s partial sum
    rounded through fp32, or the weights rounded to fp32"""
    if w_f32:
        filters = [w.astype(np.float32).astype(np.float64) for w in filters]
    acc = np.zeros((len(filters), feat.shape[0], feat.shape[1] // FLEN))
    for t, win, w in _terms(feat, filters):
        part = np.tensordot(w, win, axes=([1], [2]))
        if t == tap_f32:
            part = part.astype(np.float32).astype(np.float64)
        acc += part
    return acc


def _ref_f64(oracle, feat, filters):
    return np.stack([oracle.conv(feat, w) for w in filters])


# ---- 1. ref64 is the oracle's correlation --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 4, 5, 7, 9, 12])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref64_matches_oracle_conv(oracle, k, dtype):
    rng = np.random.default_rng(k)
    u, both = (R.U32, False) if dtype == np.float32 else (R.U64, True)
    total = R.Stats(u)
    # 1 x 1, smaller than the filter, empty, ordinary, and a non-zero channel 31 inside the map
    for (h, w, c31) in [(1, 1, 0.0), (max(k - 2, 1), 2, 0.0), (0, 5, 0.0), (3, 0, 0.0), (13, 17, 0.0), (9, 11, 0.3)]:
        feat = R.uniform_features(rng, h, w, c31=c31).astype(dtype)
        filt = [f.astype(dtype) for f in R.normal_filters(rng, [k] * 3)]
        ref, M = R.ref64(feat, filt, ksize=[k] * 3)
        assert ref.shape == (3, h, w)
        if h * w == 0:
            continue
        got = np.stack([oracle.conv(feat, f) for f in filt])
        s = R.check(got, ref, M, _K(filt[0]), u, both_rounded=both, where=f"{h}x{w}")
        R.assert_ok(s, f"k={k} {h}x{w}")
        total = total + s
        if c31:
            # channel 31 inside the map is a real channel: dropping it must show
            ref0, _ = R.ref64(np.where(np.arange(w * FLEN) % FLEN == FLEN - 1, 0, feat).astype(dtype), filt)
            assert np.abs(ref0 - ref).max() > 100 * R.bound(M, _K(filt[0]), u).max()
    assert total.rms * 10 <= total.bar, total


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref64_matches_oracle_responses_mixed_sizes(oracle, dtype):
    flat = MD.synthetic_model(seed=9, pa=[0, 1, 1, 2], nmix=3, ksize=[3, 4, 5, 7, 9, 12]).flatten()
    filters = R.model_filters(flat, dtype)
    assert sorted(set(int(k) for k in flat.filter_ksize)) == [3, 4, 5, 7, 9, 12]
    rng = np.random.default_rng(3)
    u, both = (R.U32, False) if dtype == np.float32 else (R.U64, True)
    for h, w in [(1, 1), (5, 3), (16, 21)]:
        feat = R.uniform_features(rng, h, w).astype(dtype)
        ref, M = R.ref64(feat, filters, ksize=list(flat.filter_ksize))
        got = oracle.responses(flat, feat)
        R.assert_ok(R.check(got, ref, M, _nvec(filters, "fma"), u, both_rounded=both), f"{h}x{w}")


def test_check_criteria_themselves():
    """M == 0 demands an exact 0; a non-finite response fails; the RMS merges over planes"""
    M = np.array([0.0, 1.0, 1.0])
    assert R.check(np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 2.0]), M, 800, R.U32).ok
    assert not R.check(np.array([1e-30, 1.0, 2.0]), np.array([0.0, 1.0, 2.0]), M, 800, R.U32).elem_ok
    assert not R.check(np.array([0.0, np.inf, 2.0]), np.array([0.0, 1.0, 2.0]), M, 800, R.U32).elem_ok
    s = R.check(np.array([1.0 + 2.0 ** -19]), np.array([1.0]), np.array([1.0]), 800, R.U32)
    assert s.elem_ok and not s.rms_ok
    assert (s + R.check(np.zeros(3), np.zeros(3), np.ones(3), 800, R.U32)).rms == pytest.approx(2.0 ** -20)
    # bf16 / fp16 emulations: round to nearest even
    assert R.bf16(np.float32(1.0 + 2.0 ** -8)) == 1.0 and R.bf16(np.float32(1.0 + 3 * 2.0 ** -8)) == 1.0 + 2.0 ** -6
    hi, lo = R.split_bf16(np.float32(0.1))
    assert hi + lo != hi and abs(float(hi) + float(lo) - float(np.float32(0.1))) <= 2.0 ** -17 * 0.1
    assert R.f16(np.float32(65519.0)) == 65504.0 and np.isinf(R.f16(np.float32(65520.0)))
    assert R.half_ulp_f16(1.0) == 2.0 ** -11 and R.half_ulp_f16(1e-6) == 2.0 ** -25


# ---- 2. acceptance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["fma", "mfma", "f16", "f64"])
def test_correct_mode_emulation_passes(oracle, hog_level, kind, mode):
    feat, filters = _inputs(kind, hog_level)
    if mode == "f64":
        f64 = [w.astype(np.float64) for w in filters]
        feat64 = feat.astype(np.float64)
        M = R.ref64(feat64, f64)[1]
        s = R.check(emu_f64(feat64, f64), _ref_f64(oracle, feat64, f64), M, _nvec(f64, mode), R.U64, both_rounded=True)
    else:
        ref, M = R.ref64(feat, filters, mode=mode)
        n = _nvec(filters, mode)
        if mode == "fma":
            s = R.check(emu_fma32(feat, filters), ref, M, n, R.U32)
        elif mode == "mfma":
            s = R.check(emu_split32(feat, filters), ref, M, n, R.U32)
        else:
            s = R.f16_check(emu_f16(feat, filters), ref, M, n)
    print(f"{mode} {kind}: {s}")
    R.assert_ok(s, f"{mode} {kind}")
    assert s.rms * 10 <= s.bar, s


# ---- 3. rejection -------------------------------------------------------------------------------------------------------
TAP, KSTEP, PROD_C = 12, range(16), 4          # the centre tap of 5 x 5; its first 16-channel K-step; one channel of it
MUTANTS = {
    # mfma: against the bf16x3 reference
    "mfma_no_hi_hi": ("mfma", lambda f, w: emu_split32(f, w, terms=("hl", "lh"))),
    "mfma_no_hi_lo": ("mfma", lambda f, w: emu_split32(f, w, terms=("hh", "lh"))),
    "mfma_no_lo_hi": ("mfma", lambda f, w: emu_split32(f, w, terms=("hh", "hl"))),
    "mfma_lo_dropped_on_one_tap": ("mfma", lambda f, w: emu_split32(f, w, drop_hl=lambda t, c: t == TAP)),
    "mfma_lo_dropped_on_one_kstep": ("mfma", lambda f, w: emu_split32(f, w, drop_hl=lambda t, c: t == TAP and c in KSTEP)),
    "mfma_lo_dropped_on_one_product": ("mfma", lambda f, w: emu_split32(f, w, drop_hl=lambda t, c: t == TAP and c == PROD_C)),
    "mfma_hi_only_bf16": ("mfma", lambda f, w: emu_split32(f, w, terms=("hh",))),
    # f16: against the fp16-operand reference
    "f16_operands_rounded_to_bf16": ("f16", lambda f, w: emu_f16(f, w, rnd=R.bf16)),
    # fma (fp32): against the plain reference
    "fma_one_tap_partial_through_f16": ("fma", lambda f, w: emu_fma32(f, w, tap_f16=TAP)),
    # fp64 modes: against the oracle's double responses
    "f64_one_tap_partial_through_f32": ("f64", lambda f, w: emu_f64(f, w, tap_f32=TAP)),
    "f64_weights_rounded_to_f32": ("f64", lambda f, w: emu_f64(f, w, w_f32=True)),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_rejected(oracle, hog_level, mutant, kind):
    mode, emu = MUTANTS[mutant]
    feat, filters = _inputs(kind, hog_level)
    if mode == "f64":
        # fp64 inputs that fp32 cannot hold: the weights' low bits matter
        rng = np.random.default_rng(77)
        f64 = [w.astype(np.float64) + rng.standard_normal(w.shape) * 1e-9 for w in filters]
        feat64 = feat.astype(np.float64)
        M = R.ref64(feat64, f64)[1]
        s = R.check(emu(feat64, f64), _ref_f64(oracle, feat64, f64), M, _nvec(f64, mode), R.U64, both_rounded=True)
    else:
        ref, M = R.ref64(feat, filters, mode=mode)
        got = emu(feat, filters)
        n = _nvec(filters, mode)
        s = R.f16_check(got, ref, M, n) if mode == "f16" else R.check(got, ref, M, n, R.U32)
    print(f"{mutant} {kind}: {s}")
    assert not s.ok, f"mutant {mutant} passes on {kind} inputs: {s}"
