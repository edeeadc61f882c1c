"""PBD_CONV_MFMA_ANY (5) and PBD_CONV_MFMA_F16_ANY (6): the float matrix-core convolution for every filter side 1 .. 31 and mixed
banks (csrc/pbd_kernels_conv_mfma_any.hip), through the C ABI as the other mode tests go.

  1. one-hot banks (tests/conv_any_cases.py): every tap and every channel of every side around the host's staging changes,
     EXACT equality with the emulated reference, inequality with PBD_CONV_FMA (which carries lo*lo), exact zeros where M == 0;
  2. dense banks within the bounds pinned in tests/conv_reference.py (per element and RMS bar 2^-20; nothing tuned here);
  3. an all-5 x 5 bank is the kernel and the records of modes 2 / 3: bit for bit;
  4. the detect path (staged responses of later frames; detections at 480 x 640 against the oracle within the score bound);
  5. fp16 residency of mode 6;  6. in-place model update and the latent twin;  7. refusals.

Latent detection in mode 6 masks its fp16 responses with the most negative finite half (-65504) where the other real types
write -1e10, and reports found = score > -32752 (include/pbd.h); mode 3 keeps its refusal."""
import numpy as np
import pytest

import conv_any_cases as A
import conv_reference as R
import test_gpu_conv_modes as T
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as MD
from partsbaseddetector_amd import synth

pytestmark = pytest.mark.gpu

FLEN = R.FLEN
EMU = {"any": "mfma", "any16": "f16"}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch                 # (train() and the QP use torch: it initialises the device before the library does)
    torch.cuda.init()


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.fixture(scope="module")
def L():
    from partsbaseddetector_amd import _lib
    return _lib


def _conv_mode(L, name):
    return {"any": L.CONV_MFMA_ANY, "any16": L.CONV_MFMA_F16_ANY, "fma": L.CONV_FMA, "mfma": L.CONV_MFMA, "f16": L.CONV_MFMA_F16}[name]


def pdf(det_mod, L, name, filters, feats, model=None):
    hd = det_mod.Handle((model or MD.synthetic_tiny_model()).flatten(), device=0, conv_mode=_conv_mode(L, name))
    try:
        conv = det_mod.SpatialConvolutionEngine(hd)
        conv.setFilters([np.asarray(w, np.float32) for w in filters])
        return conv.pdf([np.asarray(f, np.float32) for f in feats])
    finally:
        hd.close()


def run_pdf(det_mod, oracle, L, name, filters, feats, tag):
    """test_gpu_conv_modes.run_pdf for the new modes: the same per-level check, the same two criteria"""
    got = pdf(det_mod, L, name, filters, feats)
    total = R.Stats(R.U32)
    for f, g in zip(feats, got):
        total = total + T.check_level(oracle, name, EMU[name], R.U32, g, np.asarray(f, np.float32), filters,
                                      f"{name} {tag} level {f.shape[0]}x{f.shape[1] // FLEN}")
    print(f"[{name} {tag}] worst element {total.worst:.3g} of the bound, RMS {total.rms:.3g} = {total.rms / total.bar:.3g} of the bar "
          f"({total.count} elements)")
    R.assert_ok(total, f"{name} {tag}")
    return total


# ---- 1. one-hot banks ---------------------------------------------------------------------------------------------------------
_onehot_feats = A.onehot_features(5, A.ONEHOT_LEVELS)
_fma_cache = {}


def _fma_onehot(det_mod, L, k):
    if k not in _fma_cache:
        _fma_cache[k] = pdf(det_mod, L, "fma", A.onehot_bank(k)[0], _onehot_feats)
    return _fma_cache[k]


@pytest.mark.parametrize("name,k", [("any", k) for k in A.SIDES_BF16] + [("any16", k) for k in A.SIDES_F16])
def test_onehot_banks_are_exact(det_mod, L, name, k):
    filters, _ = A.onehot_bank(k)
    got = pdf(det_mod, L, name, filters, _onehot_feats)
    fma = _fma_onehot(det_mod, L, k)
    for feat, g, v in zip(_onehot_feats, got, fma):
        ref, M = A.onehot_ref(feat, k, EMU[name])
        want = ref.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref)
        if name == "any16":
            want = R.f16_response(want)
            assert np.array_equal(g.astype(np.float16).astype(np.float32), g)          # fp16-representable
        assert g.shape == want.shape and g.dtype == np.float32
        bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (name, k, feat.shape, len(bad), bad[:4], g[tuple(bad[0])], want[tuple(bad[0])])
        assert np.all(g[M == 0] == 0)
        # the vector mode computes the whole fp32 product (lo*lo included): another number wherever the feature is a map cell
        differs = A.onehot_differs(feat, k)
        assert differs.any() and np.all(v[differs] != g[differs]), (name, k)
        assert np.all(v[M == 0] == 0)


# ---- 2. bounds on dense banks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["any", "any16"])
@pytest.mark.parametrize("nf", [1, 31, 33, 161])
@pytest.mark.parametrize("k", [3, 4, 7, 9, 12])
def test_dense_banks_every_level_shape(det_mod, oracle, L, name, k, nf):
    rng = np.random.default_rng(4000 + 37 * k + nf)
    run_pdf(det_mod, oracle, L, name, R.normal_filters(rng, [k] * nf), T._feats(rng, T.LEVELS_SMALL, c31_level=3), f"k={k}, {nf} filters")


WIDE_LEVELS = [(1, 40), (33, 8), (9, 37), (40, 70), (0, 5)]


@pytest.mark.parametrize("name", ["any", "any16"])
@pytest.mark.parametrize("k", [18, 19, 31])
def test_wide_filters(det_mod, oracle, L, name, k):
    rng = np.random.default_rng(4100 + k)
    filters = R.normal_filters(rng, [k] * 5)
    run_pdf(det_mod, oracle, L, name, filters, T._feats(rng, WIDE_LEVELS, c31_level=2), f"k={k}, 5 filters")


MIXED = [3, 4, 5, 7, 9, 12]


@pytest.mark.parametrize("name", ["any", "any16"])
def test_mixed_bank(det_mod, oracle, L, name):
    rng = np.random.default_rng(4200)
    filters = R.normal_filters(rng, [MIXED[i % len(MIXED)] for i in range(33)])
    run_pdf(det_mod, oracle, L, name, filters, T._feats(rng, T.LEVELS_SMALL, c31_level=3), "mixed bank, 33 filters")


@pytest.mark.parametrize("name", ["any", "any16"])
def test_hog_and_cancelling_filters(det_mod, oracle, L, name):
    rng = np.random.default_rng(11)
    flat = MD.synthetic_person_model().flatten()
    feats, _ = oracle.features_pyramid(flat, synth.synthetic_frame(41, 150, 190, 3))
    feats = [np.ascontiguousarray(f) for f in feats]
    run_pdf(det_mod, oracle, L, name, R.zero_mean_filters(rng, [5] * 9 + [7] * 8), feats, "HOG features, zero-mean filters")


@pytest.mark.parametrize("name,e", [("any", 20), ("any", -20), ("any16", -20)])
def test_mixed_bank_holds_at_scale(det_mod, oracle, L, name, e):
    """features x 2^e (weights x 2^-20 when e < 0): the bound is relative.  fp16 operands have no range upwards (0.4 x 2^20 is
    past 65504), so x 2^20 is mode 5's case alone, as test_fp32_modes_hold_at_scale is mode 2's and not mode 3's; downwards
    the fp16 operands go subnormal or to zero, which the emulated reference (conv_reference.f16) does as well."""
    rng = np.random.default_rng(50 + e)
    filters = R.normal_filters(rng, [MIXED[i % len(MIXED)] for i in range(33)])
    if e < 0:
        filters = [w * np.float32(2.0 ** -20) for w in filters]
    run_pdf(det_mod, oracle, L, name, filters, T._feats(rng, T.LEVELS_SMALL, scale=2.0 ** e), f"features x 2^{e}")


# ---- 3. 5 x 5 banks are the old kernel's -------------------------------------------------------------------------------------
def _staged_and_candidates(det_mod, L, model, conv_mode, frames, frame_idx):
    det = det_mod.PartsBasedDetector(device=0, conv_mode=conv_mode, max_batch=len(frames))
    det.distributeModel(model)
    try:
        cands = det.detect_batch(frames)
        plan = det.hd.plan(*frames[0].shape[:2])
        planes = []
        for lvl in range(plan["nlevels"]):
            h, w = int(plan["feat_rows"][lvl]), int(plan["feat_cols"][lvl])
            if h * w:
                planes.append(det.hd.get_stage(L.STAGE_RESPONSES, frame_idx, lvl, h, w))
        return planes, det.hd.pack_candidates(cands)
    finally:
        det.hd.close()


@pytest.mark.parametrize("new,old", [("any", "mfma"), ("any16", "f16")])
def test_5x5_bank_equals_the_5x5_mode(det_mod, L, new, old):
    model = MD.synthetic_person_model(thresh=-1e9)           # every root is a candidate
    frames = [synth.synthetic_frame(60 + i, 96, 128, 3) for i in range(2)]
    pa, ca = _staged_and_candidates(det_mod, L, model, _conv_mode(L, new), frames, 1)
    pb, cb = _staged_and_candidates(det_mod, L, model, _conv_mode(L, old), frames, 1)
    assert len(pa) == len(pb) > 0 and len(ca) > 0
    for u, v in zip(pa, pb):
        assert u.shape == v.shape and u.tobytes() == v.tobytes()
    assert ca.tobytes() == cb.tobytes()


# ---- 4. the detect path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["any", "any16"])
def test_detect_path_responses_of_later_frames(det_mod, oracle, L, name):
    """the person_mixed model of test_gpu_conv_modes (sides 3, 4, 7): pbd_detect_batch (4 equal frames) and pbd_detect_frames
    (mixed sizes), checked as _check_staged checks the other modes"""
    model = T._model([3, 4, 7])
    flat = model.flatten()
    det = det_mod.PartsBasedDetector(device=0, conv_mode=_conv_mode(L, name), max_batch=4)
    det.distributeModel(model)
    try:
        frames = [synth.synthetic_frame(60 + i, 96, 128, 3) for i in range(4)]
        det.detect_batch(frames)
        total = R.Stats(R.U32)
        for fi in (1, 3):
            total = total + T._check_staged(det, oracle, name, EMU[name], R.U32, fi, frames[fi], flat, np.float32, 3)
        mixed = [synth.synthetic_frame(70, 77, 93, 3), synth.synthetic_frame(71, 130, 101, 3), synth.synthetic_frame(72, 64, 150, 3)]
        det.detect_frames(mixed)
        for fi in (1, 2):
            total = total + T._check_staged(det, oracle, name, EMU[name], R.U32, fi, mixed[fi], flat, np.float32, 3)
    finally:
        det.hd.close()
    print(f"[{name} detect path] worst element {total.worst:.3g} of the bound, RMS {total.rms / total.bar:.3g} of the bar ({total.count})")
    R.assert_ok(total, f"{name} detect path")


def test_detections_person_mixed_480x640(det_mod, oracle, L):
    """mode 5 against the oracle within the score bound B, exactly as test_gpu_conv_modes.test_detections_person_model_480x640
    holds fma_mixed (the oracle side is that case's)"""
    model = T._model([3, 4, 7])
    flat = model.flatten()
    im = synth.synthetic_frame(3, 480, 640, 3)
    det = det_mod.PartsBasedDetector(device=0, conv_mode=L.CONV_MFMA_ANY)
    det.distributeModel(model)
    try:
        got = det.detect(im)
    finally:
        det.hd.close()
    want = oracle.detect(flat, im, dtype=np.float32)
    feats, _ = oracle.features_pyramid(flat, im, dtype=np.float32)
    B = T._score_bound(flat, feats, "mfma", R.U32, False)
    thresh = float(flat.thresh)
    slack = lambda s: B + 64 * R.U32 * max(1.0, abs(s))
    gk = {(c.level, c.component, c.root[0], c.root[1]): c for c in got}
    wk = {(c["level"], c["component"], c["root_x"], c["root_y"]): c for c in want}
    for key, c in wk.items():
        if abs(c["score"] - thresh) > slack(c["score"])[key[0]]:
            assert key in gk, f"oracle root {key} score {c['score']} (B {B[key[0]]:.3g}) not found"
    for key, c in gk.items():
        if key not in wk:
            assert abs(c.score() - thresh) <= slack(c.score())[key[0]], f"root {key} score {c.score()} not in the oracle's"
    both = sorted(set(gk) & set(wk))
    assert both
    worst = max(abs(gk[key].score() - wk[key]["score"]) / slack(wk[key]["score"])[key[0]] for key in both)
    print(f"[any detections] {len(got)} found, {len(want)} in the oracle, {len(both)} shared; largest score difference {worst:.3g} of its bound")
    assert worst <= 1.0, worst


# ---- 5. fp16 residency in mode 6 ----------------------------------------------------------------------------------------------
def test_f16_any_responses_are_fp16_and_saturate(det_mod, oracle, L):
    """test_f16_responses_past_65520_are_infinite with a 7 x 7 bank; every response read back is an fp16 number"""
    rng = np.random.default_rng(9)
    filters = R.normal_filters(rng, [7] * 34)
    for s, f in ((1.0, 32), (-1.0, 33)):
        filters[f] = np.zeros((7, 7 * FLEN), np.float32)
        filters[f][3, 3 * FLEN + 0] = s * 60000.0                  # centre tap, channel 0; fp16-exact
    dims = [(9, 17), (33, 8), (2, 2)]
    feats = T._feats(rng, dims)
    feats[1].reshape(33, 8, FLEN)[20, 3, 0] = 2.0                 # 120000 at (20, 3) of level 1
    got = pdf(det_mod, L, "any16", filters, feats)
    assert got[1][32, 20, 3] == np.inf and got[1][33, 20, 3] == -np.inf
    assert np.isfinite(np.delete(got[1].reshape(34, -1), 20 * 8 + 3, axis=1)).all()
    total = R.Stats(R.U32)
    for f, g in zip(feats, got):
        with np.errstate(over="ignore"):
            assert np.array_equal(g.astype(np.float16).astype(np.float32), g)
        total = total + T.check_level(oracle, "any16", "f16", R.U32, g, f, filters, f"f16 overflow {f.shape}")
    R.assert_ok(total, "any16 overflow")


def test_f16_any_dp_min_rounds_its_input(det_mod, oracle, L):
    """the assertion of test_gpu_parity.test_mfma_f16_dp_min_rounds_its_input, on a 3 x 3 model in mode 6"""
    model = MD.synthetic_model(seed=3, pa=[0, 1, 1, 2], nmix=2, ksize=[3], name="tiny3")
    flat = model.flatten()
    hd = det_mod.Handle(flat, device=0, conv_mode=L.CONV_MFMA_F16_ANY)
    try:
        dp = det_mod.DynamicProgram(hd)
        rng = np.random.default_rng(12)
        dims = [(21, 30), (9, 14)]
        scores = [rng.standard_normal((flat.nfilters, h, w)).astype(np.float32) * 1.7 for h, w in dims]      # not fp16-representable
        f16 = lambda a: a.astype(np.float16).astype(np.float32)
        assert not np.array_equal(scores[0], f16(scores[0]))
        Ix, Iy, Ik, rootv, rooti = dp.min(scores)
        for l in range(len(dims)):
            for c in range(flat.ncomponents):
                oIx, oIy, oIk, orv, ori = oracle.dp_min(flat, c, f16(scores[l]))
                assert np.array_equal(rootv[l][c].view(np.uint32), orv.view(np.uint32))
                assert np.array_equal(rooti[l][c], ori)
                p0, p1 = flat.part_offset[c], flat.part_offset[c + 1]
                for gp in range(p0 + 1, p1):
                    par = p0 + flat.parentid[gp]
                    for m in range(flat.mix_offset[par + 1] - flat.mix_offset[par]):
                        sl = flat.ptr_slot[gp] + m
                        assert np.array_equal(Ik[l][sl], oIk[sl]) and np.array_equal(Ix[l][sl], oIx[sl]) and np.array_equal(Iy[l][sl], oIy[sl])
                unrounded = oracle.dp_min(flat, c, scores[l])[3]
                assert not np.array_equal(rootv[l][c], unrounded)
    finally:
        hd.close()


# ---- 6. model update and latent twin ------------------------------------------------------------------------------------------
from test_gpu_model_update import LOW, assert_equal, handle, mixed_model, new_vector, observe, rounded, two_frames  # noqa: E402

UPDATE_MODELS = {"9-8": lambda: mixed_model([9, 8], 2), "3-4-7": lambda: mixed_model([3, 4, 7], 3)}


@pytest.mark.parametrize("name", ["any", "any16"])
@pytest.mark.parametrize("which", sorted(UPDATE_MODELS))
def test_update_equals_fresh_handle(L, name, which):
    mode = _conv_mode(L, name)
    model = UPDATE_MODELS[which]()
    flat = model.flatten()
    frames = two_frames((140, 120))
    hd = handle(model, np.float32, mode)
    fresh = None
    try:
        before = observe(hd, frames)
        w = new_vector(hd, flat)
        hd.set_model_vector(w)
        assert hd.model_vector().tobytes() == rounded(w, flat, np.float32).tobytes()
        got = observe(hd, frames)
        fresh = handle(model.from_vector(w), np.float32, mode)
        assert fresh.model_vector().tobytes() == hd.model_vector().tobytes()
        assert_equal(got, observe(fresh, frames))
        assert got[0].tobytes() != before[0].tobytes()          # and the update changed what is detected
        a, b = hd.current_model().flatten(), fresh.current_model().flatten()
        assert a.filters_f32.tobytes() == b.filters_f32.tobytes() and np.array_equal(a.biasw, b.biasw) and np.array_equal(a.defw, b.defw)
    finally:
        hd.close()
        if fresh:
            fresh.close()


@pytest.mark.parametrize("name", ["any", "any16"])
@pytest.mark.parametrize("which", sorted(UPDATE_MODELS))
def test_latent_twin_is_a_plain_detection_of_the_unique_model(det_mod, L, which, name):
    """overlap -1 masks nothing: after pbd_detect_latent every stage equals that of a unique_model handle of the same mode
    after a plain detect, before and after an in-place update (the twin follows its handle)"""
    from test_gpu_examples import records
    model = UPDATE_MODELS[which]()
    flat = model.flatten()
    im = synth.synthetic_frame(61, 140, 120)
    boxes = [[[20, 16, 60, 56]] * flat.max_parts]
    hd = det_mod.Handle(model, device=0, conv_mode=_conv_mode(L, name), max_candidates=1 << 12)
    try:
        for rnd in range(2):
            current = hd.current_model()
            plain = det_mod.Handle(E.unique_model(current), device=0, conv_mode=_conv_mode(L, name), max_candidates=1 << 18)
            try:
                hd.detect_latent([im], boxes, -1.0)
                records(plain, [im])
                p = hd.plan(*im.shape[:2])
                for lvl in range(p["nlevels"]):
                    shape = int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl])
                    if shape[0] * shape[1] == 0:
                        continue
                    for s in (L.STAGE_FEATURES, L.STAGE_RESPONSES, L.STAGE_ROOTV, L.STAGE_ROOTI):
                        u, v = hd.get_stage(s, 0, lvl, *shape), plain.get_stage(s, 0, lvl, *shape)
                        assert u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes(), (rnd, lvl, s)
            finally:
                plain.close()
            if rnd == 0:
                hd.set_model_vector(new_vector(hd, flat, seed=5))
    finally:
        hd.close()


MASK = {"any": np.float32(E.MASKED), "any16": np.float32(-65504.0)}       # mode 6: the most negative finite half
FOUND = {"any": -5e9, "any16": -32752.0}


@pytest.mark.parametrize("name", ["any", "any16"])
def test_latent_mask_on_the_modes_own_responses(det_mod, L, name):
    """the pattern of test_gpu_latent_hard.test_mask_in_other_convolution_modes on the 9 / 12 / 5 sizes model: every level's
    masked responses == where(keep, a unique_model handle's unmasked responses of the same mode, the mode's mask value), the
    record is the first maximum of the root planes, found = 1; with overlap = inf everything is masked and found = 0"""
    import latent_hard_cases as LH
    from test_gpu_examples import records
    case = LH.sizes_case("9_12_5")
    mode = _conv_mode(L, name)
    im, boxes = case.frames[0], case.boxes[0]
    uflat = E.unique_model(case.model).flatten()
    hd = det_mod.Handle(case.model, device=0, conv_mode=mode, max_candidates=1 << 12)
    plain = det_mod.Handle(E.unique_model(case.model), device=0, conv_mode=mode, max_candidates=1 << 16)
    try:
        records(plain, [im])
        rec, found = hd.detect_latent([im], [boxes], case.overlap)
        p = hd.plan(*im.shape[:2])
        kept, best = 0, None
        for lvl in range(p["nlevels"]):
            rows, cols = int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl])
            if rows * cols == 0:
                continue
            want = plain.get_stage(L.STAGE_RESPONSES, 0, lvl, rows, cols)
            ys, xs = np.mgrid[0:rows, 0:cols]
            keep = {}
            for gp in range(uflat.part_offset[0], uflat.part_offset[-1]):
                part = gp - int(uflat.part_offset[np.searchsorted(uflat.part_offset, gp, side="right") - 1])
                for gm in range(uflat.mix_offset[gp], uflat.mix_offset[gp + 1]):
                    key = (part, int(uflat.filter_ksize[gm]))
                    if key not in keep:
                        keep[key] = E.overlap_passes(E.part_rects(xs, ys, key[1], p["scales"][lvl], np.float32), boxes[part],
                                                     LH.widened(case.overlap))
                    want[gm][~keep[key]] = MASK[name]
            got = hd.get_stage(L.STAGE_RESPONSES, 0, lvl, rows, cols)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), lvl
            kept += int((want != MASK[name]).sum())
            rv = hd.get_stage(L.STAGE_ROOTV, 0, lvl, rows, cols)
            i = int(np.argmax(rv))
            if best is None or rv.flat[i] > best[4]:
                c, y, x = np.unravel_index(i, rv.shape)
                best = (lvl, int(c), int(x), int(y), rv.flat[i])
        assert kept > 0 and found[0] == 1 and best[4] > FOUND[name]
        assert tuple(int(t) for t in rec[0, :5]) == (0, best[1], best[0], best[2], best[3])
        assert rec[0, 5:6].view(np.float32)[0].tobytes() == np.float32(best[4]).tobytes()
        rec, found = hd.detect_latent([im], [boxes], np.inf)
        assert found[0] == 0 and rec[0, 5:6].view(np.float32)[0] < FOUND[name]
        lvl = p["nlevels"] // 2
        got = hd.get_stage(L.STAGE_RESPONSES, 0, lvl, int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl]))
        assert got.size and np.all(got == MASK[name])
    finally:
        plain.close()
        hd.close()


@pytest.mark.parametrize("name", ["any", "any16"])
def test_failed_set_filters_keeps_the_old_bank(det_mod, L, name):
    """a 33 x 33 bank is outside 1 .. 31 in every mode: the old (mixed) bank still answers, bit for bit"""
    rng = np.random.default_rng(8)
    hd = det_mod.Handle(MD.synthetic_tiny_model().flatten(), device=0, conv_mode=_conv_mode(L, name))
    try:
        conv = det_mod.SpatialConvolutionEngine(hd)
        good = R.normal_filters(rng, [3, 4, 7, 3, 7])
        conv.setFilters(good)
        feat = rng.random((17, 29 * 32), dtype=np.float32) * 0.4
        before = conv.pdf([feat])[0]
        with pytest.raises(det_mod.PbdError) as e:
            conv.setFilters([rng.standard_normal((33, 33 * 32)).astype(np.float32) for _ in range(4)])
        assert e.value.code == -2
        conv._nfilters = len(good)
        after = conv.pdf([feat])[0]
        assert before.shape == (5, 17, 29) and np.array_equal(before.view(np.uint32), after.view(np.uint32))
        # a 5 x 5 bank (the records of modes 2 / 3) and back to the mixed one: each bank answers as a fresh handle's
        conv.setFilters(R.normal_filters(rng, [5] * 3))
        conv.pdf([feat])
        conv.setFilters(good)
        assert np.array_equal(conv.pdf([feat])[0].view(np.uint32), before.view(np.uint32))
    finally:
        hd.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(det_mod, L):
    flat = MD.synthetic_tiny_model().flatten()
    for mode in (L.CONV_MFMA_ANY, L.CONV_MFMA_F16_ANY):
        with pytest.raises(det_mod.PbdError) as e:
            det_mod.Handle(flat, device=0, conv_mode=mode, real_type=L.REAL_F64)
        assert e.value.code == -2 and "PBD_CONV_MFMA_F64" in str(e.value)
    hd = det_mod.Handle(flat, device=0, conv_mode=L.CONV_MFMA)
    try:
        conv = det_mod.SpatialConvolutionEngine(hd)
        with pytest.raises(det_mod.PbdError) as e:
            conv.setFilters(R.normal_filters(np.random.default_rng(1), [3] * 4))
        assert e.value.code == -2
    finally:
        hd.close()
    hd = det_mod.Handle(flat, device=0, conv_mode=L.CONV_MFMA_F16)          # mode 3 keeps refusing latent detection
    try:
        with pytest.raises(det_mod.PbdError) as e:
            hd.detect_latent([synth.synthetic_frame(61, 72, 96)], [[[20, 16, 60, 56]] * flat.max_parts], 0.3)
        assert e.value.code == -2 and "PBD_CONV_MFMA_F16" in str(e.value)
    finally:
        hd.close()


# ---- 8. train() in the new modes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["any", "any16"])
def test_train_runs_in_the_new_modes(L, name):
    """train() mines latent positives (pbd_detect_latent) and negatives in the mode it is given: one iteration of the latent
    case of tests/train_cases.py finds its positives and returns a trained model, in mode 6 as in mode 5"""
    import train_cases as TC
    from partsbaseddetector_amd import train as TR
    model, pos, neg, kw = TC.latent_case()
    got_model, info = TR.train(model, pos, neg, 0, dtype=np.float32, conv_mode=_conv_mode(L, name), **kw)
    assert info["lb"] > 0 and len(info["notfound"]) < len(pos) and sum(info["numpositives"]) > 0
    assert got_model.to_vector(np.float32).tobytes() != model.to_vector(np.float32).tobytes()
