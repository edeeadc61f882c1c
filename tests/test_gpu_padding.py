"""The padded pyramid on the device (pbd_set_padding) against its numpy rule (partsbaseddetector_amd/
padding.py, on the oracle): records, features, every convolution mode, the uint8 / int16 pointer threshold, every entry point,
the staged seam, examples, latent positives, suppression, refusals and state.  Comparisons are of bytes unless said otherwise."""
import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import padding as P
from partsbaseddetector_amd.detector import Candidate, PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
DTYPES = [np.float32, np.float64]
PADS = [(0, 0), (2, 2), (1, 3), (7, 5)]
COUNTS = {(0, 0): 446, (2, 2): 986, (1, 3): 996, (7, 5): 2672}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def frame():
    return synth.synthetic_frame(5, 48, 64)


def tiny(thresh=-1.0):
    return M.synthetic_tiny_model(thresh=thresh)


_refs = {}


def ref(model, im, pad, dtype, walk="reference", tag="tiny"):
    """detect_ref, computed once per case and shared"""
    key = (tag, float(model.thresh), im.shape, pad, np.dtype(dtype).name, walk)
    if key not in _refs:
        _refs[key] = P.detect_ref(model, im, pad[0], pad[1], dtype, walk)
    return _refs[key]


def key(c):
    return (c.frame, c.level, c.component, c.root, np.float32(c.score()).tobytes(), np.asarray(c.parts, np.int32).tobytes())


def keys(cands):
    return [key(c) for c in cands]


def same_as_ref(got, want, frame_id=0):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (g.frame, g.level, g.component, g.root[1], g.root[0]) == (frame_id, w["level"], w["component"], w["root_y"], w["root_x"])
        assert np.float32(g.score()).tobytes() == np.float32(w["score"]).tobytes()
        assert np.array_equal(g.parts, w["parts"]), (g.level, g.root, g.parts, w["parts"])


def padded_detector(model, pad, dtype=np.float32, **kw):
    det = detector.PartsBasedDetector(device=0, dtype=dtype, **kw)
    det.setPadding(*pad)
    det.distributeModel(model)
    return det


# ---- 1. records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_records_equal_the_rule(frame, dtype, walk):
    model = tiny()
    det = detector.PartsBasedDetector(device=0, dtype=dtype)
    det.setWalk(walk)
    det.distributeModel(model)
    fresh = keys(det.detect(frame))
    for pad in PADS:
        det.setPadding(*pad)
        got = det.detect(frame)
        assert len(got) == COUNTS[pad]
        same_as_ref(got, ref(model, frame, pad, dtype, walk))
        if pad != (0, 0):       # parts the unpadded detector cannot place: left of the frame
            scales = det.features_.scales()
            assert any(np.any(c.parts[:, 0] < -float(scales[c.level]) - 1) for c in got)
    det.setPadding(0)
    assert keys(det.detect(frame)) == fresh
    det.hd.close()


# ---- 2. features ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sbin", [4, 8])
@pytest.mark.parametrize("kind", ["bgr8", "grey16"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_planes_are_pad_features_of_the_unpadded_ones(dtype, kind, sbin):
    model = M.synthetic_model(seed=11, pa=[0, 1, 1], nmix=2, ksize=5, sbin=sbin, interval=3, thresh=1e9, name="pad-feat")
    rows, cols = (75, 101) if sbin == 4 else (139, 170)
    if kind == "bgr8":
        im = synth.synthetic_frame(9, rows, cols, 3)
    else:
        im = (synth.synthetic_frame(9, rows, cols, 1).astype(np.uint16).reshape(rows, cols, 1) * 257 + 31).astype(np.uint16)
    pad = (3, 2)
    bare = detector.Handle(model, device=0, real_type=REAL[dtype])
    padded = detector.Handle(model, device=0, real_type=REAL[dtype])
    try:
        padded.set_padding(*pad)
        want = [P.pad_features(f, pad[0], pad[1]) for f in detector.HOGFeatures(bare).pyramid(im)]
        got = detector.HOGFeatures(padded).pyramid(im)
        plan, plan0 = padded.plan(rows, cols), bare.plan(rows, cols)
        assert len(got) == len(want) == plan["nlevels"] >= 4
        for l, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape == (plan["feat_rows"][l], plan["feat_cols"][l] * 32)
            assert (plan["feat_rows"][l], plan["feat_cols"][l]) == (plan0["feat_rows"][l] + 2 * pad[1], plan0["feat_cols"][l] + 2 * pad[0])
            assert g.tobytes() == w.tobytes(), l
            stage = padded.get_stage(_lib.STAGE_FEATURES, 0, l, int(plan["feat_rows"][l]), int(plan["feat_cols"][l]))
            assert stage.tobytes() == w.tobytes(), l
            cells = g.reshape(g.shape[0], -1, 32)
            assert not np.any(np.signbit(cells[:pad[1], :, :31])) and np.all(cells[:pad[1], :, 31] == 1)
    finally:
        bare.close()
        padded.close()


# ---- 3. every convolution mode ----------------------------------------------------------------------------------------------
def _conv_check(oracle, model, dtype, mode, im, pad):
    flat = model.flatten()
    padded = detector.Handle(model, device=0, real_type=REAL[dtype], conv_mode=mode)
    bare = detector.Handle(model, device=0, real_type=REAL[dtype], conv_mode=mode)
    try:
        padded.set_padding(*pad)
        assert padded.detect(np.ascontiguousarray(im)) == []
        plan = padded.plan(im.shape[0], im.shape[1])
        shapes = [(int(r), int(c)) for r, c in zip(plan["feat_rows"], plan["feat_cols"])]
        ofeats, _ = oracle.features_pyramid(flat, im, dtype)
        feats = [P.pad_features(f, pad[0], pad[1]) for f in ofeats]
        for l, (r, c) in enumerate(shapes):
            assert padded.get_stage(_lib.STAGE_FEATURES, 0, l, r, c).tobytes() == feats[l].tobytes(), l
        got = [padded.get_stage(_lib.STAGE_RESPONSES, 0, l, r, c) for l, (r, c) in enumerate(shapes)]
        want = detector.SpatialConvolutionEngine(bare).pdf(feats)
        for l, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (mode, l)
            if mode == _lib.CONV_EXACT:
                assert g.tobytes() == oracle.responses(flat, feats[l]).tobytes(), l
    finally:
        padded.close()
        bare.close()


@pytest.mark.parametrize("dtype,mode", [(np.float32, m) for m in (0, 1, 2, 3, 5, 6)] + [(np.float64, m) for m in (0, 1, 4)])
def test_every_convolution_mode_on_padded_planes(oracle, dtype, mode):
    _conv_check(oracle, tiny(1e9), dtype, mode, synth.synthetic_frame(7, 61, 83), (3, 2))


@pytest.mark.parametrize("mode", [0, 5])
def test_mixed_filter_sizes_on_padded_planes(oracle, mode):
    model = M.synthetic_model(seed=17, pa=[0, 1, 1], nmix=2, ksize=[7, 3], interval=3, thresh=1e9, name="pad-7-3")
    assert sorted(set(int(k) for k in model.flatten().filter_ksize)) == [3, 7]
    _conv_check(oracle, model, np.float32, mode, synth.synthetic_frame(7, 61, 83), (3, 3))


# ---- 4. the uint8 / int16 position planes at a longest padded side of 256 ---------------------------------------------------
@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("shape", [(40, 1008), (1008, 40)])
def test_pointer_width_threshold(oracle, shape, pad):
    model = tiny(0.9)
    flat = model.flatten()
    im = synth.synthetic_frame(13, shape[0], shape[1])
    det = padded_detector(model, (pad, pad))
    try:
        plan = det.hd.plan(*shape)
        assert max(int(plan["feat_rows"].max()), int(plan["feat_cols"].max())) == (256 if pad == 3 else 258)
        want = ref(model, im, (pad, pad), np.float32, tag="ptr8")
        assert len(want) > 50
        same_as_ref(det.detect(im), want)
        feats, _ = oracle.features_pyramid(flat, im)
        resp = [oracle.responses(flat, P.pad_features(f, pad, pad)) for f in feats]
        Ix, Iy, Ik, rootv, rooti = det.dp_.min(resp)
        for l, r in enumerate(resp):
            for c in range(flat.ncomponents):
                oIx, oIy, oIk, orv, ori = oracle.dp_min(flat, c, r)
                assert rootv[l][c].tobytes() == orv.tobytes() and np.array_equal(rooti[l][c], ori), l
                for gp in range(flat.part_offset[c] + 1, flat.part_offset[c + 1]):
                    par = flat.part_offset[c] + flat.parentid[gp]
                    for m in range(flat.mix_offset[par + 1] - flat.mix_offset[par]):
                        s = flat.ptr_slot[gp] + m
                        assert np.array_equal(Ix[l][s], oIx[s]) and np.array_equal(Iy[l][s], oIy[s]) and np.array_equal(Ik[l][s], oIk[s]), (l, s)
    finally:
        det.hd.close()


# ---- 5. entry points -----------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_single_call():
    import torch
    model = tiny(0.2)
    pad = (2, 3)
    det = padded_detector(model, pad, max_batch=4)
    try:
        frames = [synth.synthetic_frame(21, 60, 84), synth.synthetic_frame(22, 60, 84)]
        single = [keys(det.detect(f)) for f in frames]
        assert all(len(s) > 20 for s in single)
        same_as_ref(det.detect(frames[0]), ref(model, frames[0], pad, np.float32, tag="entry"))

        def per_frame(cands, n):
            return [[key(c)[1:] for c in cands if c.frame == f] for f in range(n)]

        want = [[k[1:] for k in s] for s in single]
        assert per_frame(det.detect_batch(frames), 2) == want
        det.submit_batch(frames)
        assert per_frame(det.wait_batch(), 2) == want
        mixed = [frames[0], synth.synthetic_frame(23, 52, 44), synth.synthetic_frame(24, 71, 97)]
        want3 = [[key(c)[1:] for c in det.detect(f)] for f in mixed]
        assert per_frame(det.detect_frames(mixed), 3) == want3
        # regions of one device image, read in place
        big = synth.synthetic_frame(25, 120, 160)
        rects = [(10, 8, 84, 60), (60, 50, 44, 52)]
        t = torch.from_numpy(big).to("cuda:0")
        wantr = [[key(c)[1:] for c in det.detect(np.ascontiguousarray(big[y:y + h, x:x + w]))] for x, y, w, h in rects]
        assert per_frame(det.detect_regions(t, rects), 2) == wantr
        # the union of a two-rank level shard is the unsharded list
        full = keys(det.detect(frames[0]))
        union = []
        for rank in range(2):
            det.hd.set_level_shard(rank, 2)
            plan = det.hd.plan(60, 84)
            mine = det.detect(frames[0])
            assert all(plan["feat_rows"][c.level] > 0 for c in mine)
            union += mine
        det.hd.set_level_shard(0, 1)
        union.sort(key=lambda c: (c.level, c.component, c.root[1], c.root[0]))
        assert keys(union) == full
    finally:
        det.hd.close()


# ---- 6. the staged seam --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_staged_calls_give_the_fused_records(frame, dtype):
    model = tiny()
    pad = (1, 3)
    det = padded_detector(model, pad, dtype)
    bare = detector.Handle(model, device=0, real_type=REAL[dtype])
    try:
        fused = keys(det.detect(frame))
        plan, plan0 = det.hd.plan(48, 64), bare.plan(48, 64)
        assert np.array_equal(plan["img_rows"], plan0["img_rows"]) and np.array_equal(plan["scales"], plan0["scales"])
        assert np.array_equal(plan["feat_rows"], plan0["feat_rows"] + 2 * pad[1])
        assert np.array_equal(plan["feat_cols"], plan0["feat_cols"] + 2 * pad[0])
        feats = det.features_.pyramid(frame)
        resp = det.convolution_engine_.pdf(feats)
        det.dp_.min(resp)
        staged = det.dp_.argmin(det.features_.scales())
        assert keys(staged) == fused
    finally:
        det.hd.close()
        bare.close()


# ---- 7. examples ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_examples_follow_the_padded_planes(frame, dtype):
    model = tiny()
    flat = model.flatten()
    pad = (2, 2)
    det = padded_detector(model, pad, dtype)
    det.setWalk("argmax")
    try:
        cands = det.detect(frame)
        rec = det.hd.pack_candidates(cands)
        hdr, vals = det.hd.examples(rec)
        maps = E.FrameMaps(flat, frame, dtype, walk="argmax", pad=pad)
        want_h, want_v = E.examples_of_records(flat, [maps], rec, 0, dtype, walk="argmax")
        assert np.array_equal(hdr, want_h)
        assert vals.tobytes() == want_v.tobytes()
        assert any(r[3] < pad[0] or r[4] < pad[1] for r in rec)          # roots in the pad were among them
        w = det.hd.model_vector()
        got = E.dot(hdr, vals, w)
        bound = E.rounding_bound(flat, hdr, vals, w, dtype)
        plan = det.hd.plan(48, 64)
        rootv = {}
        for i, r in enumerate(rec):
            l = int(r[2])
            if l not in rootv:
                rootv[l] = det.hd.get_stage(_lib.STAGE_ROOTV, 0, l, int(plan["feat_rows"][l]), int(plan["feat_cols"][l]))
            score = float(rootv[l][int(r[1]), int(r[4]), int(r[3])])     # the root's score in T (the record's is rounded to float)
            assert abs(got[i] - score) <= bound[i], (i, got[i], score, bound[i])
    finally:
        det.hd.close()


@pytest.mark.parametrize("walk", ["reference", "argmax"])
def test_part_scores_in_plane_coordinates(frame, walk):
    from partsbaseddetector_amd import partscores as S
    model = tiny(0.0)
    flat = model.flatten()
    pad = (2, 2)
    det = padded_detector(model, pad)
    det.setWalk(walk)
    try:
        rec = det.hd.pack_candidates(det.detect(frame))
        assert len(rec) > 50 and any(r[3] < pad[0] or r[4] < pad[1] for r in rec)
        status, place, scores = det.hd.part_scores(rec)
        maps = E.FrameMaps(flat, frame, np.float32, walk=walk, pad=pad)
        want = S.scores_of_records(flat, [maps], rec, 0, np.float32, walk=walk)
        assert np.array_equal(status, want[0]) and np.array_equal(place, want[1])
        assert scores.tobytes() == want[2].tobytes()
    finally:
        det.hd.close()


# ---- 8. latent positives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_latent_positives_with_a_box_half_outside(dtype, walk):
    model = tiny(-100.0)
    pad = (2, 2)
    det = padded_detector(model, pad, dtype, max_batch=2)
    det.setWalk(walk)
    try:
        frames = [synth.synthetic_frame(11, 40, 56), synth.synthetic_frame(12, 52, 44)]
        found0 = det.detect(frames[0])
        inside = max(found0, key=lambda c: c.score())
        # ground truth half outside the frame: the root part's box shifted so that its left half lies left of column 0
        x, y, w, h = (int(v) for v in inside.parts[0])
        shift = x + w // 2
        boxes = [[(int(a) - shift, int(b), int(a) - shift + int(c), int(b) + int(d)) for a, b, c, d in inside.parts]]
        best1 = max(det.detect(frames[1]), key=lambda c: c.score())
        boxes.append([(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in best1.parts])
        assert boxes[0][0][0] < 0 < boxes[0][0][2]
        rec, found = det.hd.detect_latent(frames, boxes, 0.3, None)
        assert list(found) == [1, 1]
        for f, im in enumerate(frames):
            want = E.latent_search(model, im, boxes[f], 0.3, None, dtype, walk, pad=pad)
            r = rec[f]
            assert (r[0], r[1], r[2], r[3], r[4]) == (f, want["component"], want["level"], want["root_x"], want["root_y"]), f
            assert r[5:6].view(np.float32)[0].tobytes() == np.float32(want["score"]).tobytes()
            assert r[6] == len(want["parts"]) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want["parts"])
            assert bool(found[f]) == want["found"]
        assert np.any(rec[0, 8:8 + 4 * rec[0, 6]].reshape(-1, 4)[:, 0] < 0)
    finally:
        det.hd.close()


# ---- 9. suppression ------------------------------------------------------------------------------------------------------
def test_suppression_on_a_padded_handle(frame):
    model = tiny(0.0)
    det = padded_detector(model, (2, 2))
    try:
        raw = det.detect(frame)
        assert len(raw) > 50 and any(np.any(c.parts[:, 0] < 0) for c in raw)
        want = list(raw)
        Candidate.sort(want)
        Candidate.nonMaximaSuppression(frame.shape[:2], want, float(np.float32(0.3)))
        det.hd.set_nms(0.3)
        got = det.detect(frame)
        assert 0 < len(got) < len(raw)
        assert keys(got) == keys(want)
    finally:
        det.hd.close()


# ---- 10. refusals and state ----------------------------------------------------------------------------------------------
def test_refusals_and_state(frame):
    model = tiny(0.2)
    det = detector.PartsBasedDetector(device=0, max_batch=2)
    det.distributeModel(model)
    hd = det.hd
    try:
        for bad in [(-1, 0), (0, -1), (32, 0), (0, 32), (1 << 20, 1)]:
            with pytest.raises(PbdError) as e:
                hd.set_padding(*bad)
            assert e.value.code == -1, bad
        hd.set_padding(31, 31)
        hd.set_padding(0, 0)
        # in flight
        det.submit_batch([frame])
        with pytest.raises(PbdError) as e:
            hd.set_padding(2, 2)
        assert e.value.code == -5
        det.wait_batch()
        # depth pruning, in both orders
        hd.set_padding(2, 2)
        with pytest.raises(PbdError) as e:
            hd.set_depth_prune(500.0, 0.5, 0.3)
        assert e.value.code == -2
        hd.set_padding(0, 0)
        hd.set_depth_prune(500.0, 0.5, 0.3)
        with pytest.raises(PbdError) as e:
            hd.set_padding(2, 2)
        assert e.value.code == -2
        hd.set_depth_prune(None)
        hd.set_padding(2, 2)
        # max-marginals and marginal poses on a padded result
        cands = det.detect(frame)
        assert len(cands) > 0
        with pytest.raises(PbdError) as e:
            hd.max_marginals(0)
        assert e.value.code == -2
        with pytest.raises(PbdError) as e:
            hd.marginal_poses(np.array([[0, 0, 0, -1, 1, 1]], np.int32))
        assert e.value.code == -2
        # a call that changes nothing leaves the resident result; one that changes a value drops it
        plan = hd.plan(48, 64)
        r0, c0 = int(plan["feat_rows"][0]), int(plan["feat_cols"][0])
        rec = hd.pack_candidates(cands)
        before = hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0)
        hd.set_padding(2, 2)
        assert hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0).tobytes() == before.tobytes()
        assert len(hd.examples(rec)[0]) == len(rec)
        hd.set_padding(2, 1)
        for reader in (lambda: hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0), lambda: hd.get_stage(_lib.STAGE_FEATURES, 0, 0, r0, c0),
                       lambda: hd.examples(rec), lambda: hd.part_scores(rec), lambda: hd.dp_argmin(plan["scales"])):
            with pytest.raises(PbdError) as e:
                reader()
            assert e.value.code == -5
        # a model update keeps the setting
        hd.set_padding(2, 2)
        want = keys(det.detect(frame))
        det.updateModel(hd.model_vector())
        assert keys(det.detect(frame)) == want
        same_as_ref(det.detect(frame), ref(model, frame, (2, 2), np.float32, tag="state"))
        # the detector keeps it across distributeModel, and refuses depth pruning beside it before a handle exists
        det.setPadding(2)
        det.distributeModel(model)
        assert keys(det.detect(frame)) == want
        with pytest.raises(PbdError) as e:
            det.setDepthPrune(500.0, 0.5, 0.3)
        assert e.value.code == -2
        assert model.full_padding() == (2, 2)
    finally:
        det.hd.close()
