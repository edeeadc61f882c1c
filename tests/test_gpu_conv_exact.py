"""Every exact-convolution kernel variant (PBD_CONV_EXACT: k_conv3<false, NW>, k_conv_generic<float|double, false, 5|0>,
csrc/pbd_kernels_conv.hip) against the oracle, bit for bit, on EVERY level and every filter of built banks and level lists
(tests/conv_exact_cases.py).  No tolerance appears here.

What each test reaches is asserted from host logic in tests/test_conv_exact_cpu.py, which also ties the oracle to a plain numpy
statement of the arithmetic and measures how many responses change under another tap / channel order or a fused multiply-add:

  test_conv3_banks_pdf[n]              k_conv3<false>, c31_zero == 0 (channel 31 computed), units of 8 / 6 / 4 / 2, partial units
                                       of the odd banks, tiles of 1 / 2 / 3 segments over up to three levels, one unit per blockIdx.y
  test_conv3_large_cover_pdf           >= 1024 workgroups: units_per_block == nunits
  test_conv3_inside_mixed_bank[t]      the fmap store of k_conv3 (f32) beside a generic class in the same call; f64: both generic
  test_generic_sizes_pdf[t-K]          k_conv_generic<R, false, 0> at every cblock, <double, false, 5>, ragged filter groups,
                                       even sizes, maps smaller than the filter
  test_generic_large_cover_pdf[t]      groups_per_block == ngroups
  test_zero_negative_zero_and_subnormal[t]   +0 responses by their bits, subnormals kept
  test_fused_channel31_every_level[shape]    skip31 and the channel-31 table: all 36 reachable cases, interior and border tiles
  test_fused_batch_frames_cross_tiles  tiles whose segments lie in two frames, frame0 + frame addressing
  test_fused_mixed_size_call           the virtual-frame plan of pbd_detect_frames through k_conv3
  test_fused_double_handle_every_level k_conv_generic<double, false, 5> on library HOG
"""
import numpy as np
import pytest

import conv_exact_cases as X
from partsbaseddetector_amd import model as MD

pytestmark = pytest.mark.gpu

TYPES = {"f32": "float32", "f64": "float64"}
_WANT = {}


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.fixture(scope="module")
def L():
    from partsbaseddetector_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def engines(det_mod, L):
    """one exact-mode handle per real type for the pdf tests (setFilters replaces the bank)"""
    flat = MD.synthetic_tiny_model().flatten()
    hds = {t: det_mod.Handle(flat, device=0, conv_mode=L.CONV_EXACT, real_type=L.REAL_F32 if t == "f32" else L.REAL_F64)
           for t in TYPES}
    yield {t: det_mod.SpatialConvolutionEngine(hd) for t, hd in hds.items()}
    for hd in hds.values():
        hd.close()


def want_of(oracle, key, feats, filters):
    """the oracle's responses of a case, computed once per process and frozen"""
    if key not in _WANT:
        out = tuple(X.oracle_responses(oracle, f, filters) for f in feats)
        for a in out:
            a.setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def check_pdf(engines, oracle, t, key, feats, filters):
    conv = engines[t]
    dt = np.dtype(TYPES[t])
    assert all(f.dtype == dt for f in feats) and all(w.dtype == dt for w in filters)
    conv.setFilters(list(filters))
    got = conv.pdf(list(feats))
    want = want_of(oracle, key, feats, filters)
    assert len(got) == len(feats)
    for l, (f, g, w) in enumerate(zip(feats, got, want)):
        assert g.dtype == dt and g.shape == w.shape == (len(filters), f.shape[0], f.shape[1] // X.FLEN)
        same = X.bits(g) == X.bits(w)
        assert same.all(), (f"{key} level {l} {w.shape}: {int((~same).sum())} of {same.size} responses differ, filters "
                            f"{sorted(set(np.nonzero(~same)[0].tolist()))[:12]}")
    return got


# ---- pdf: k_conv3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.CONV3_BANKS)
def test_conv3_banks_pdf(engines, oracle, n):
    feats = X.level_features("conv3", "float32")
    assert any(f.size and f.reshape(f.shape[0], -1, X.FLEN)[:, :, 31].any() for f in feats)      # channel 31 is computed
    check_pdf(engines, oracle, "f32", ("conv3", n), feats, X.bank((5,) * n, "float32"))


def test_conv3_large_cover_pdf(engines, oracle):
    check_pdf(engines, oracle, "f32", ("conv3 large",), X.level_features("large", "float32"),
              X.bank((5,) * X.LARGE_BANK_CONV3, "float32", seed=1))


@pytest.mark.parametrize("t", sorted(TYPES))
def test_conv3_inside_mixed_bank(engines, oracle, t):
    check_pdf(engines, oracle, t, ("mixed", t), X.level_features("conv3", TYPES[t]), X.bank(X.mixed_sizes(), TYPES[t]))


# ---- pdf: k_conv_generic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,K,n", [("f32", K, n) for K, n in X.GENERIC_BANKS] + [("f64", K, n) for K, n in X.GENERIC_BANKS_F64])
def test_generic_sizes_pdf(engines, oracle, t, K, n):
    check_pdf(engines, oracle, t, ("generic", t, K, n), X.level_features("generic", TYPES[t]), X.bank((K,) * n, TYPES[t]))


@pytest.mark.parametrize("t", sorted(TYPES))
def test_generic_large_cover_pdf(engines, oracle, t):
    K, n = X.LARGE_BANK_GENERIC
    check_pdf(engines, oracle, t, ("generic large", t), X.level_features("large", TYPES[t]), X.bank((K,) * n, TYPES[t], seed=1))


@pytest.mark.parametrize("t", sorted(TYPES))
def test_zero_negative_zero_and_subnormal(engines, oracle, t):
    """f32: K = 5 is k_conv3, K = 3 k_conv_generic<float>; f64: k_conv_generic<double> with and without compile-time taps"""
    dtn = TYPES[t]
    tiny = np.finfo(np.dtype(dtn)).tiny
    for k in (5, 3):
        feats, filters = X.zero_case(k, dtn)
        got = check_pdf(engines, oracle, t, ("zero", t, k), feats, filters)
        for f, g in zip(feats, got):
            if not f.any():
                assert not X.bits(g).any(), "every response of an all-zero level is +0 by its bits"
        feats, filters = X.subnormal_case(k, dtn)
        got = check_pdf(engines, oracle, t, ("subnormal", t, k), feats, filters)
        assert all((np.abs(g) < tiny).all() for g in got) and sum(int(np.count_nonzero(g)) for g in got) > sum(g.size for g in got) // 2


# ---- the fused detect path ------------------------------------------------------------------------------------------------
def check_staged(det, L, oracle, flat, frame_idx, im, dt):
    """features and responses of every level of one frame of the resident result against the oracle of that frame alone"""
    plan = det.hd.plan(im.shape[0], im.shape[1])
    dims = [(int(h), int(w)) for h, w in zip(plan["feat_rows"], plan["feat_cols"])]
    assert dims == X.plan_dims(oracle, im.shape[:2], flat.sbin, flat.interval)            # the reach counts are of these maps
    feats, _ = oracle.features_pyramid(flat, im, dtype=dt)
    assert len(feats) == plan["nlevels"] and all(h * w > 0 for h, w in dims)
    for lvl, (h, w) in enumerate(dims):
        f = det.hd.get_stage(L.STAGE_FEATURES, frame_idx, lvl, h, w)
        assert f.dtype == np.dtype(dt) and np.array_equal(X.bits(f), X.bits(np.ascontiguousarray(feats[lvl]).reshape(f.shape)))
        assert not f.reshape(h, w, X.FLEN)[:, :, 31].any()
        got = det.hd.get_stage(L.STAGE_RESPONSES, frame_idx, lvl, h, w)
        want = oracle.responses(flat, f)
        same = X.bits(got) == X.bits(want)
        assert got.dtype == want.dtype and same.all(), (f"frame {frame_idx} {im.shape[:2]} level {lvl} ({h} x {w}): "
                                                        f"{int((~same).sum())} of {same.size} responses differ")
    return dims


def fused_detector(det_mod, dt=np.float32, max_batch=1):
    det = det_mod.PartsBasedDetector(device=0, max_batch=max_batch, dtype=dt)
    det.distributeModel(X.fused_model())
    return det


@pytest.mark.parametrize("shape", X.FUSED_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fused_channel31_every_level(det_mod, L, oracle, shape):
    flat = X.fused_model().flatten()
    det = fused_detector(det_mod)
    try:
        im = X.fused_frame(500 + shape[0], shape)
        assert det.detect(im) == []
        check_staged(det, L, oracle, flat, 0, im, np.float32)
    finally:
        det.hd.close()


def test_fused_batch_frames_cross_tiles(det_mod, L, oracle):
    flat = X.fused_model().flatten()
    det = fused_detector(det_mod, max_batch=3)
    try:
        frames = [X.fused_frame(600 + i, X.BATCH_SHAPE) for i in range(3)]
        assert det.detect_batch(frames) == []
        for i, im in enumerate(frames):
            check_staged(det, L, oracle, flat, i, im, np.float32)
    finally:
        det.hd.close()


def test_fused_mixed_size_call(det_mod, L, oracle):
    flat = X.fused_model().flatten()
    det = fused_detector(det_mod, max_batch=3)
    try:
        frames = [X.fused_frame(700 + i, s) for i, s in enumerate(X.MIXED_SHAPES)]
        assert det.detect_frames(frames) == []
        for i, im in enumerate(frames):
            check_staged(det, L, oracle, flat, i, im, np.float32)
    finally:
        det.hd.close()


def test_fused_double_handle_every_level(det_mod, L, oracle):
    flat = X.fused_model().flatten()
    assert all(int(k) == 5 for k in flat.filter_ksize)
    det = fused_detector(det_mod, dt=np.float64)
    try:
        for shape in (X.FUSED_SHAPES[0], X.FUSED_SHAPES[3]):
            im = X.fused_frame(800 + shape[0], shape)
            assert det.detect(im) == []
            check_staged(det, L, oracle, flat, 0, im, np.float64)
    finally:
        det.hd.close()
