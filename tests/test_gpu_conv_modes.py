"""Every inexact convolution mode against a float64 reference (tests/conv_reference.py), with bounds relative to the scale
M = sum |w| |f| of each response and an RMS criterion that catches a systematically missing term:

  PBD_CONV_FMA float 5 x 5 (k_conv3<true>), float other / mixed sizes (k_conv_generic<float, true>), double (k_conv_generic
  <double, true>, the compile-time 5 x 5 path and the runtime-K path), PBD_CONV_MFMA (bf16 hi/lo split), PBD_CONV_MFMA_F16
  (fp16 operands and responses), PBD_CONV_MFMA_F64.

Through pbd_conv_pdf on level shapes that exercise the tile covers (sides 1 .. 130, maps smaller than the filter, empty levels,
all in one call), the filter counts around the kernels' tile / pass sizes, real HOG, uniform and scaled features and zero-mean
filters; through the detect path's staged responses of frames f > 0 of pbd_detect_batch and pbd_detect_frames; and the
detections on the person model at 480 x 640 against the oracle, within the score bound B the response bounds imply.
The bounds were derived and pinned on the CPU (tests/test_conv_bounds_cpu.py); they are not tuned here."""
import numpy as np
import pytest

import conv_reference as R
from partsbaseddetector_amd import model as MD
from partsbaseddetector_amd import synth

pytestmark = pytest.mark.gpu

FLEN = R.FLEN
SIDES = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
# every side as a height and as a width, square and paired with another side; maps smaller than any filter; empty levels
LEVELS = [(s, s) for s in SIDES] + [(h, SIDES[(i + 5) % len(SIDES)]) for i, h in enumerate(SIDES)] + [(0, 5), (7, 0)]
# the same sides at a fraction of the cells (where the reference is the single-threaded oracle): large paired with small
LEVELS_SMALL = list(zip(SIDES, SIDES[::-1])) + [(0, 3)]

REPORT = {}


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.fixture(scope="module")
def L():
    from partsbaseddetector_amd import _lib
    return _lib


def _mode(L, name):
    """conv_mode, real type, the emulation of conv_reference, accumulation unit roundoff"""
    return {"fma": (L.CONV_FMA, L.REAL_F32, "fma", R.U32), "mfma": (L.CONV_MFMA, L.REAL_F32, "mfma", R.U32),
            "f16": (L.CONV_MFMA_F16, L.REAL_F32, "f16", R.U32), "fma64": (L.CONV_FMA, L.REAL_F64, "f64", R.U64),
            "mfma64": (L.CONV_MFMA_F64, L.REAL_F64, "f64", R.U64)}[name]


def _record(name, s):
    REPORT[name] = REPORT[name] + s if name in REPORT else s
    t = REPORT[name]
    print(f"[{name}] worst element {t.worst:.3g} of the bound, RMS {t.rms:.3g} = {t.rms / t.bar:.3g} of the bar ({t.count} elements)")


def _nvec(filters, emu):
    return np.array([R.products(emu, w.shape[0] * w.shape[0] * FLEN) for w in filters], np.float64)[:, None, None]


def check_level(oracle, name, emu, u, got, feat, filters, where):
    """one level's responses (F, H, W) of a mode against its reference; returns Stats"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    assert got.shape == (len(filters), H, W), (got.shape, where)
    if H * W == 0:
        return R.Stats(u)
    n = _nvec(filters, emu)
    if u == R.U64:
        # the oracle's own double responses (bit-exact with the exact GPU path), rounded as well: doubled bound
        feat = np.ascontiguousarray(feat, np.float64)
        ref = np.stack([oracle.conv(feat, np.ascontiguousarray(w, np.float64)) for w in filters])
        M = R.ref64(feat, filters)[1]
        return R.check(got, ref, M, n, u, both_rounded=True, where=where)
    ref, M = R.ref64(feat, filters, mode=emu)
    if emu == "f16":
        return R.f16_check(got, ref, M, n, where=where)
    return R.check(got, ref, M, n, u, where=where)


def run_pdf(det_mod, oracle, L, name, filters, feats, tag):
    conv_mode, real, emu, u = _mode(L, name)
    dt = np.float32 if real == L.REAL_F32 else np.float64
    hd = det_mod.Handle(MD.synthetic_tiny_model().flatten(), device=0, conv_mode=conv_mode, real_type=real)
    try:
        conv = det_mod.SpatialConvolutionEngine(hd)
        conv.setFilters([np.asarray(w, dt) for w in filters])
        got = conv.pdf([np.asarray(f, dt) for f in feats])
    finally:
        hd.close()
    total = R.Stats(u)
    for f, g in zip(feats, got):
        total = total + check_level(oracle, name, emu, u, g, np.asarray(f, dt), [np.asarray(w, dt) for w in filters],
                                    f"{name} {tag} level {f.shape[0]}x{f.shape[1] // FLEN}")
    _record(name, total)
    R.assert_ok(total, f"{name} {tag}")
    return total


def _feats(rng, dims, scale=1.0, c31_level=None):
    out = [R.uniform_features(rng, h, w) * np.float32(scale) for h, w in dims]
    if c31_level is not None and out[c31_level].size:          # a non-zero channel 31 inside the map
        h, w = dims[c31_level]
        out[c31_level].reshape(h, w, FLEN)[:, :, 31] = 0.25 * scale
    return out


@pytest.fixture(scope="module")
def hog_levels(oracle):
    """real HOG levels of one frame (person model's pyramid), channel 31 = 0"""
    flat = MD.synthetic_person_model().flatten()
    feats, _ = oracle.features_pyramid(flat, synth.synthetic_frame(41, 150, 190, 3))
    return [np.ascontiguousarray(f) for f in feats]


# ---- matrix-core modes: 5 x 5 float banks around the 32-filter M-tiles and the 160-filter passes ------------------------------
MFMA_COUNTS = [1, 31, 32, 33, 159, 160, 161, 321]


@pytest.mark.parametrize("name", ["mfma", "f16"])
@pytest.mark.parametrize("nf", MFMA_COUNTS)
def test_matrix_core_modes_every_level_shape(det_mod, oracle, L, name, nf):
    rng = np.random.default_rng(1000 + nf)
    filters = R.normal_filters(rng, [5] * nf)
    dims = LEVELS if nf in (33, 161) else LEVELS_SMALL
    run_pdf(det_mod, oracle, L, name, filters, _feats(rng, dims, c31_level=3), f"{nf} filters, uniform features")


@pytest.mark.parametrize("name", ["mfma", "f16"])
def test_matrix_core_modes_hog_and_cancelling_filters(det_mod, oracle, L, hog_levels, name):
    rng = np.random.default_rng(7)
    run_pdf(det_mod, oracle, L, name, R.normal_filters(rng, [5] * 161), hog_levels, "HOG features")
    run_pdf(det_mod, oracle, L, name, R.zero_mean_filters(rng, [5] * 33), hog_levels, "HOG features, zero-mean filters")
    run_pdf(det_mod, oracle, L, name, R.zero_mean_filters(rng, [5] * 33), _feats(rng, LEVELS_SMALL),
            "uniform features, zero-mean filters")


@pytest.mark.parametrize("e", [20, -20])
@pytest.mark.parametrize("name,ks", [("mfma", [5]), ("fma", [5]), ("fma", [3]), ("fma", [3, 4, 5, 7, 9, 12])])
def test_fp32_modes_hold_at_scale(det_mod, oracle, L, name, ks, e):
    """the bound is relative: features scaled by 2^e (and the weights by 2^-20 when e < 0: products near 2^-40) must pass as
    unit-scale ones do (MFMA takes 5 x 5 banks only)"""
    rng = np.random.default_rng(50 + e)
    filters = R.normal_filters(rng, [ks[i % len(ks)] for i in range(33)])
    if e < 0:
        filters = [w * np.float32(2.0 ** -20) for w in filters]
    run_pdf(det_mod, oracle, L, name, filters, _feats(rng, LEVELS_SMALL, scale=2.0 ** e), f"features x 2^{e}")


def test_f16_responses_past_65520_are_infinite(det_mod, oracle, L):
    """unit-scale inputs, and two filters whose response at one cell is past the fp16 range: +inf and -inf there"""
    rng = np.random.default_rng(9)
    filters = R.normal_filters(rng, [5] * 34)
    for s, f in ((1.0, 32), (-1.0, 33)):
        filters[f] = np.zeros((5, 5 * FLEN), np.float32)
        filters[f][2, 2 * FLEN + 0] = s * 60000.0                  # centre tap, channel 0; fp16-exact
    dims = [(9, 17), (33, 8), (2, 2)]
    feats = _feats(rng, dims)
    feats[1].reshape(33, 8, FLEN)[20, 3, 0] = 2.0                 # 120000 at (20, 3) of level 1
    conv_mode, real, emu, u = _mode(L, "f16")
    hd = det_mod.Handle(MD.synthetic_tiny_model().flatten(), device=0, conv_mode=conv_mode, real_type=real)
    try:
        conv = det_mod.SpatialConvolutionEngine(hd)
        conv.setFilters(filters)
        got = conv.pdf(feats)
    finally:
        hd.close()
    assert got[1][32, 20, 3] == np.inf and got[1][33, 20, 3] == -np.inf
    assert np.isfinite(np.delete(got[1].reshape(34, -1), 20 * 8 + 3, axis=1)).all()
    total = R.Stats(u)
    for f, g in zip(feats, got):
        total = total + check_level(oracle, "f16", emu, u, g, f, filters, f"f16 overflow {f.shape}")
    _record("f16", total)
    R.assert_ok(total, "f16 overflow")


# ---- FMA float / double and MFMA_F64: the generic kernels over filter sizes and counts --------------------------------------
GENERIC = [(3, 33), (4, 9), (7, 8), (9, 7), (12, 1), ("mixed", 33)]


def _bank(rng, k, nf):
    ks = [3, 4, 5, 7, 9, 12] if k == "mixed" else [k]
    return R.normal_filters(rng, [ks[i % len(ks)] for i in range(nf)])


@pytest.mark.parametrize("k,nf", [(5, 1), (5, 9), (5, 33), (5, 156)] + GENERIC)
def test_fma_float(det_mod, oracle, L, k, nf):
    """5 x 5 runs k_conv3<true>; every other size (and the mixed bank) k_conv_generic<float, true>"""
    rng = np.random.default_rng(300 + nf + (k if isinstance(k, int) else 99))
    run_pdf(det_mod, oracle, L, "fma", _bank(rng, k, nf), _feats(rng, LEVELS, c31_level=4), f"k={k}, {nf} filters")


@pytest.mark.parametrize("name", ["fma64", "mfma64"])
@pytest.mark.parametrize("k,nf", [(5, 1), (5, 33)] + GENERIC)
def test_fp64_modes(det_mod, oracle, L, name, k, nf):
    """FMA double: k = 5 takes the compile-time-tap path of k_conv_generic<double, true>, other sizes the runtime-K path"""
    rng = np.random.default_rng(700 + nf + (k if isinstance(k, int) else 99))
    filters = [w.astype(np.float64) + rng.standard_normal(w.shape) * 1e-9 for w in _bank(rng, k, nf)]   # not fp32-exact
    cost = sum(w.shape[0] ** 2 for w in filters)
    dims = LEVELS if cost <= 300 else LEVELS_SMALL
    feats = [f.astype(np.float64) + rng.random(f.shape) * 1e-9 * (f != 0) for f in _feats(rng, dims, c31_level=2)]
    run_pdf(det_mod, oracle, L, name, filters, feats, f"k={k}, {nf} filters")


def test_fp64_modes_hog_and_cancelling_filters(det_mod, oracle, L, hog_levels):
    rng = np.random.default_rng(11)
    feats = [f.astype(np.float64) for f in hog_levels[::3]]
    for name in ("fma64", "mfma64"):
        run_pdf(det_mod, oracle, L, name, [w.astype(np.float64) for w in R.zero_mean_filters(rng, [5] * 9 + [7] * 8)], feats,
                "HOG features, zero-mean filters")


# ---- the detect path: staged responses of frames f > 0 ------------------------------------------------------------------
DETECT_CFG = {
    "fma": ("fma", None), "fma_mixed": ("fma", [3, 4, 7]), "fma64": ("fma64", None), "fma64_mixed": ("fma64", [3, 4, 7]),
    "mfma": ("mfma", None), "f16": ("f16", None), "mfma64": ("mfma64", None),
}


def _model(ks):
    """the person model, or its layout with filters of the sizes ks (thresh 21.9: ~100 roots on the 480 x 640 frame, as
    PERSON_THRESH gives the 5 x 5 model)"""
    if ks is None:
        return MD.synthetic_person_model()
    return MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=ks, thresh=21.9, name="person_mixed")


def _check_staged(det, oracle, name, emu, u, frame_idx, im, flat, dt, every=1):
    plan = det.hd.plan(im.shape[0], im.shape[1])
    feats, _ = oracle.features_pyramid(flat, im, dtype=dt)
    filters = R.model_filters(flat, dt)
    total = R.Stats(u)
    for lvl in range(0, plan["nlevels"], every):
        h, w = int(plan["feat_rows"][lvl]), int(plan["feat_cols"][lvl])
        if h * w == 0:
            continue
        f = det.hd.get_stage(L_STAGE_FEATURES, frame_idx, lvl, h, w)
        assert np.array_equal(f, feats[lvl]), (name, frame_idx, lvl)
        got = det.hd.get_stage(L_STAGE_RESPONSES, frame_idx, lvl, h, w)
        total = total + check_level(oracle, name, emu, u, got, feats[lvl], filters, f"{name} frame {frame_idx} level {lvl}")
    return total


L_STAGE_FEATURES, L_STAGE_RESPONSES = 0, 1


@pytest.mark.parametrize("cfg", sorted(DETECT_CFG))
def test_detect_path_responses_of_later_frames(det_mod, oracle, L, cfg):
    """pbd_detect_batch (max_batch 4, equal frames) and pbd_detect_frames (mixed sizes): the responses of frames 1.. read
    each kernel's frame offset"""
    assert (L_STAGE_FEATURES, L_STAGE_RESPONSES) == (L.STAGE_FEATURES, L.STAGE_RESPONSES)
    name, ks = DETECT_CFG[cfg]
    conv_mode, real, emu, u = _mode(L, name)
    dt = np.float32 if real == L.REAL_F32 else np.float64
    model = _model(ks)
    flat = model.flatten()
    det = det_mod.PartsBasedDetector(device=0, conv_mode=conv_mode, max_batch=4, dtype=dt)
    det.distributeModel(model)
    every = 1 if dt == np.float32 and ks is None else 3          # the single-threaded oracle is the fp64 reference
    try:
        frames = [synth.synthetic_frame(60 + i, 96, 128, 3) for i in range(4)]
        det.detect_batch(frames)
        total = R.Stats(u)
        for fi in (1, 3):
            total = total + _check_staged(det, oracle, name, emu, u, fi, frames[fi], flat, dt, every)
        mixed = [synth.synthetic_frame(70, 77, 93, 3), synth.synthetic_frame(71, 130, 101, 3), synth.synthetic_frame(72, 64, 150, 3)]
        det.detect_frames(mixed)
        for fi in (1, 2):
            total = total + _check_staged(det, oracle, name, emu, u, fi, mixed[fi], flat, dt, every)
    finally:
        det.hd.close()
    _record(name, total)
    R.assert_ok(total, f"{cfg} detect path")


# ---- detections at 480 x 640 against the oracle, within the score bound B ---------------------------------------------------
def _score_bound(flat, feats, emu, u, both):
    """B[level] = sum over the model's filters of the largest per-element response bound on that level: a root score is a
    sum of one response per part (through max / min operations, which do not widen an error), so it errs by at most that"""
    filters = R.model_filters(flat, np.float32)
    n = _nvec(filters, emu)[:, 0, 0]
    B = []
    for f in feats:
        H, W = f.shape[0], f.shape[1] // FLEN
        if H * W == 0:
            B.append(0.0)
            continue
        Mmax = np.zeros(len(filters))
        for k in sorted(set(w.shape[0] for w in filters)):
            ids = [i for i, w in enumerate(filters) if w.shape[0] == k]
            wk = np.abs(np.stack([filters[i].reshape(k, k, FLEN) for i in ids]))
            P = np.abs(R.padded(f.astype(np.float32), k))
            M = R._corr(P, wk, H, W)              # float32 is enough for a bound's scale
            Mmax[ids] = M.reshape(len(ids), -1).max(axis=1)
        B.append(float(np.sum(R.bound(Mmax, n, u, both_rounded=both))))
    return np.array(B)


@pytest.mark.parametrize("cfg", ["fma", "fma_mixed", "fma64", "mfma"])
def test_detections_person_model_480x640(det_mod, oracle, L, cfg):
    name, ks = DETECT_CFG[cfg]
    conv_mode, real, emu, u = _mode(L, name)
    dt = np.float32 if real == L.REAL_F32 else np.float64
    model = _model(ks)
    flat = model.flatten()
    im = synth.synthetic_frame(3, 480, 640, 3)
    det = det_mod.PartsBasedDetector(device=0, conv_mode=conv_mode, dtype=dt)
    det.distributeModel(model)
    try:
        got = det.detect(im)
    finally:
        det.hd.close()
    want = oracle.detect(flat, im, dtype=dt)
    feats, _ = oracle.features_pyramid(flat, im, dtype=dt)
    B = _score_bound(flat, feats, emu, u, u == R.U64)
    thresh = float(flat.thresh)
    # scores cross the ABI as float: both sides round once more, and the dynamic program's own float additions (a few per
    # part) differ once its inputs do
    slack = lambda s: B + 64 * R.U32 * max(1.0, abs(s))
    gk = {(c.level, c.component, c.root[0], c.root[1]): c for c in got}
    wk = {(c["level"], c["component"], c["root_x"], c["root_y"]): c for c in want}
    for key, c in wk.items():
        if abs(c["score"] - thresh) > slack(c["score"])[key[0]]:
            assert key in gk, f"{cfg}: oracle root {key} score {c['score']} (B {B[key[0]]:.3g}) not found"
    for key, c in gk.items():
        if key not in wk:
            assert abs(c.score() - thresh) <= slack(c.score())[key[0]], f"{cfg}: root {key} score {c.score()} not in the oracle's"
    both = sorted(set(gk) & set(wk))
    assert both, cfg
    worst = 0.0
    same_parts = 0
    for key in both:
        d = abs(gk[key].score() - wk[key]["score"])
        worst = max(worst, d / slack(wk[key]["score"])[key[0]])
        same_parts += int(np.array_equal(gk[key].parts, wk[key]["parts"]))
    print(f"[{cfg} detections] {len(got)} found, {len(want)} in the oracle, {len(both)} shared; largest score difference "
          f"{worst:.3g} of its bound (B up to {B.max():.3g}); identical part placement {same_parts}/{len(both)}")
    assert worst <= 1.0, worst
