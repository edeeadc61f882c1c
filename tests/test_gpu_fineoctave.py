"""The fine octave on the device (pbd_set_fine_octave) against its numpy rule (partsbaseddetector_amd/
fineoctave.py, on the oracle): the features of every level and input path, records, the uint8 / int16 position planes, every
entry point, the readers of a resident result, the plan report, refusals and state, and the planted half-size object.
Comparisons are of bytes unless said otherwise."""
import numpy as np
import pytest

import fineoctave_cases as cases
from partsbaseddetector_amd import _lib, detector, gridnms, synth, topk
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import fineoctave as F
from partsbaseddetector_amd import marginals as MG
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import Candidate, PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
DTYPES = [np.float32, np.float64]


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


def ref(model, im, dtype, walk="reference", pad=(0, 0), fine=True, tag="tiny"):
    """detect_ref, computed once per case and shared"""
    k = (tag, float(model.thresh), im.shape, pad, np.dtype(dtype).name, walk, fine)
    if k not in _refs:
        _refs[k] = F.detect_ref(model, im, fine, pad[0], pad[1], dtype, walk)
    return _refs[k]


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


def fine_detector(model, dtype=np.float32, **kw):
    det = detector.PartsBasedDetector(device=0, dtype=dtype, **kw)
    det.setFineOctave(True)
    det.distributeModel(model)
    return det


# ---- 1. features of every level, every input path ---------------------------------------------------------------------------
# frames at sbin 4 (scaled with the bin size): the plain one; odd sizes (visible area beyond the image, clamped reads); a fine
# block grid of 35 x 67 (ragged last tile of the fused kernel in both directions); whole tiles, several per grid dimension
FRAMES = [(48, 64), (51, 77), (70, 134), (96, 160)]


def _image(kind, seed, rows, cols):
    if kind == "bgr8":
        return synth.synthetic_frame(seed, rows, cols, 3)
    if kind == "grey16":
        return (synth.synthetic_frame(seed, rows, cols, 1).astype(np.uint16).reshape(rows, cols, 1) * 257 + 31).astype(np.uint16)
    base = synth.synthetic_frame(seed, rows, cols, 3).astype(np.float32)
    return np.ascontiguousarray(base * np.float32(0.731) + synth.synthetic_frame(seed + 1, rows, cols, 3).astype(np.float32) / np.float32(64))


@pytest.mark.parametrize("sbin", [4, 6, 8])
@pytest.mark.parametrize("kind", ["bgr8", "grey16", "bgr32f"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_features_of_every_level_are_the_rules(dtype, kind, sbin):
    model = M.synthetic_model(seed=11, pa=[0, 1, 1], nmix=2, ksize=5, sbin=sbin, interval=3, thresh=1e9, name="fine-feat")
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype])
    try:
        hd.set_fine_octave(True)
        for i, (r4, c4) in enumerate(FRAMES):
            rows, cols = r4 * sbin // 4, c4 * sbin // 4
            im = _image(kind, 9 + i, rows, cols)
            want, scales = F.features_pyramid(flat, im, dtype)
            ir, ic, fr, fc, psc, nf = F.plan(rows, cols, sbin, model.interval)
            plan = hd.plan(rows, cols)
            assert nf == 3 and plan["nlevels"] == len(want) == len(ir) >= nf + 4
            assert np.array_equal(plan["img_rows"], ir) and np.array_equal(plan["img_cols"], ic)
            assert np.array_equal(plan["feat_rows"], fr) and np.array_equal(plan["feat_cols"], fc)
            assert plan["scales"].tobytes() == psc.tobytes() == scales.tobytes()
            got = detector.HOGFeatures(hd).pyramid(im)
            for l, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape == (fr[l], fc[l] * 32), (rows, cols, l)
                assert g.tobytes() == w.tobytes(), (rows, cols, l, np.argwhere(g != w)[:4])
            # a fine level owns no image: it returns the one of its base level
            for l in range(nf):
                a = np.empty((int(ir[l]), int(ic[l]), im.shape[2]), im.dtype)
                b = np.empty_like(a)
                hd.get_pyramid_image(0, l, a)
                hd.get_pyramid_image(0, nf + l, b)
                assert a.tobytes() == b.tobytes(), l
        if sbin == 4:
            assert max(fr[0], fc[0]) > 2 * 16 and (fr[0] + 2) % 16 == 0 and (fc[0] + 2) % 16 == 0      # (96, 160): 48 x 80 blocks
    finally:
        hd.close()


@pytest.mark.parametrize("sbin", [4, 8])
def test_two_pass_form_on_8_bit_frames_gives_the_fused_kernels_bytes(sbin):
    """8-bit BGR, T = float takes the fused kernel at both bin sizes; forced onto the two-pass form (one pass 1 over the shared
    images, the ranged pass 2 per bin size) the planes are the same bytes, with the octave on and off"""
    model = M.synthetic_model(seed=11, pa=[0, 1, 1], nmix=2, ksize=5, sbin=sbin, interval=3, thresh=1e9, name="fine-feat")
    flat = model.flatten()
    hd = detector.Handle(model, device=0)
    try:
        hd.set_debug_option(_lib.HOG_TWO_PASS, 1)
        for fine in (True, False):
            hd.set_fine_octave(fine)
            for i, (r4, c4) in enumerate(FRAMES[1:3]):
                im = _image("bgr8", 9 + i, r4 * sbin // 4, c4 * sbin // 4)
                want, _ = F.features_pyramid(flat, im, np.float32, fine)
                got = detector.HOGFeatures(hd).pyramid(im)
                assert len(got) == len(want)
                for l, (g, w) in enumerate(zip(got, want)):
                    assert g.tobytes() == w.tobytes(), (fine, im.shape, l)
        for bad in (2, -1):
            with pytest.raises(PbdError) as e:
                hd.set_debug_option(_lib.HOG_TWO_PASS, bad)
            assert e.value.code == -1
        hd.set_debug_option(_lib.HOG_TWO_PASS, 0)
    finally:
        hd.close()


# ---- 2. records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_records_equal_the_rule(frame, dtype, walk):
    model = tiny()
    det = detector.PartsBasedDetector(device=0, dtype=dtype)
    det.setWalk(walk)
    det.distributeModel(model)
    try:
        fresh = keys(det.detect(frame))
        same_as_ref(det.detect(frame), ref(model, frame, dtype, walk, fine=False))
        det.setFineOctave(True)
        got = det.detect(frame)
        want = ref(model, frame, dtype, walk)
        same_as_ref(got, want)
        assert len(got) > len(fresh) and {c.level for c in got} >= set(range(5))
        assert keys([c for c in got if c.level >= 5]) == [(k[0], k[1] + 5) + k[2:] for k in fresh]
        for pad in [(2, 2), (1, 3)]:
            det.setPadding(*pad)
            same_as_ref(det.detect(frame), ref(model, frame, dtype, walk, pad))
        det.setPadding(0)
        det.setFineOctave(False)
        assert keys(det.detect(frame)) == fresh
    finally:
        det.hd.close()


# ---- 3. the uint8 / int16 position planes: the fine level alone crosses 256 ------------------------------------------------------
@pytest.mark.parametrize("cols", [516, 520])
@pytest.mark.parametrize("transposed", [False, True])
def test_position_plane_edge(oracle, cols, transposed):
    model = tiny(0.9)
    flat = model.flatten()
    shape = (cols, 40) if transposed else (40, cols)
    im = synth.synthetic_frame(13, shape[0], shape[1])
    det = fine_detector(model)
    try:
        plan = det.hd.plan(*shape)
        nf = 5
        side = 256 if cols == 516 else 258
        assert max(int(plan["feat_rows"][0]), int(plan["feat_cols"][0])) == side == max(int(plan["feat_rows"].max()), int(plan["feat_cols"].max()))
        assert max(int(plan["feat_rows"][nf]), int(plan["feat_cols"][nf])) == (127 if cols == 516 else 128)
        want = ref(model, im, np.float32, tag="ptr8")
        assert len(want) > 50
        same_as_ref(det.detect(im), want)
        feats, _ = F.features_pyramid(flat, im)
        for l, f in enumerate(feats):
            r, c = int(plan["feat_rows"][l]), int(plan["feat_cols"][l])
            rootv = det.hd.get_stage(_lib.STAGE_ROOTV, 0, l, r, c)
            rooti = det.hd.get_stage(_lib.STAGE_ROOTI, 0, l, r, c)
            resp = oracle.responses(flat, f)
            for comp in range(flat.ncomponents):
                _, _, _, orv, ori = oracle.dp_min(flat, comp, resp)
                assert rootv[comp].tobytes() == orv.tobytes() and np.array_equal(rooti[comp], ori), l
    finally:
        det.hd.close()


# ---- 4. one call equals many ---------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_single_call():
    import torch
    model = tiny(0.2)
    det = fine_detector(model, max_batch=4)
    try:
        frames = [synth.synthetic_frame(21, 60, 84), synth.synthetic_frame(22, 60, 84)]
        single = [keys(det.detect(f)) for f in frames]
        assert all(len(s) > 20 for s in single)
        same_as_ref(det.detect(frames[0]), ref(model, frames[0], np.float32, tag="entry"))

        def per_frame(cands, n):
            return [[key(c)[1:] for c in cands if c.frame == f] for f in range(n)]

        want = [[k[1:] for k in s] for s in single]
        assert per_frame(det.detect_batch(frames), 2) == want
        det.submit_batch(frames)
        assert per_frame(det.wait_batch(), 2) == want
        mixed = [frames[0], synth.synthetic_frame(23, 52, 44), synth.synthetic_frame(24, 71, 97)]
        want3 = [[key(c)[1:] for c in det.detect(f)] for f in mixed]
        assert all(any(k[0] < 5 for k in w) for w in want3)                # fine-level records in every frame
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
            assert all(plan["feat_rows"][c.level] > 0 for c in mine) and 0 < len(mine) < len(full)
            union += mine
        det.hd.set_level_shard(0, 1)
        union.sort(key=lambda c: (c.level, c.component, c.root[1], c.root[0]))
        assert keys(union) == full
    finally:
        det.hd.close()


@pytest.mark.parametrize("kind", ["grey16", "bgr32f"])
def test_mixed_sizes_on_the_two_pass_path(kind):
    """the gradient planes of a mixed-size call's shared images are written once (the reference levels' table) and read by both
    bin sizes"""
    model = tiny(0.2)
    det = fine_detector(model, max_batch=4)
    try:
        ims = [_image(kind, 31 + i, r, c) for i, (r, c) in enumerate([(60, 84), (52, 44), (71, 97)])]
        want = [[key(c)[1:] for c in det.detect(im)] for im in ims]
        same_as_ref(det.detect(ims[2]), ref(model, ims[2], np.float32, tag=kind))
        got = det.detect_frames(ims)
        assert [[key(c)[1:] for c in got if c.frame == f] for f in range(3)] == want
    finally:
        det.hd.close()


# ---- 5. the readers of a fine-octave result --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_examples_of_fine_level_records(frame, dtype):
    model = tiny()
    flat = model.flatten()
    det = fine_detector(model, dtype)
    det.setWalk("argmax")
    try:
        cands = det.detect(frame)
        rec = det.hd.pack_candidates(cands)
        assert sum(1 for r in rec if r[2] < 5) > 50
        hdr, vals = det.hd.examples(rec)
        maps = E.FrameMaps(flat, frame, dtype, walk="argmax", fine=True)
        want_h, want_v = E.examples_of_records(flat, [maps], rec, 0, dtype, walk="argmax")
        assert np.array_equal(hdr, want_h)
        assert vals.tobytes() == want_v.tobytes()
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
def test_part_scores_of_fine_level_records(frame, walk):
    from partsbaseddetector_amd import partscores as S
    model = tiny(0.0)
    flat = model.flatten()
    det = fine_detector(model)
    det.setWalk(walk)
    try:
        rec = det.hd.pack_candidates(det.detect(frame))
        assert sum(1 for r in rec if r[2] < 5) > 50
        status, place, scores = det.hd.part_scores(rec)
        maps = E.FrameMaps(flat, frame, np.float32, walk=walk, fine=True)
        want = S.scores_of_records(flat, [maps], rec, 0, np.float32, walk=walk)
        assert np.array_equal(status, want[0]) and np.array_equal(place, want[1])
        assert scores.tobytes() == want[2].tobytes()
    finally:
        det.hd.close()


@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_latent_positives_of_half_the_templates_size(dtype, walk):
    model = tiny(-100.0)
    det = fine_detector(model, dtype, max_batch=2)
    det.setWalk(walk)
    try:
        frames = [synth.synthetic_frame(11, 40, 56), synth.synthetic_frame(12, 52, 44)]
        boxes = []
        for im in frames:       # ground truth: the parts of the best detection on fine level 0 -- boxes of half the template's size
            best = max((c for c in det.detect(im) if c.level == 0), key=lambda c: c.score())
            boxes.append([(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in best.parts])
        side = boxes[0][0][2] - boxes[0][0][0]
        assert side <= 5 * 2            # 5 cells of 2 pixels; the template is 5 cells of 4
        rec, found = det.hd.detect_latent(frames, boxes, 0.6, None)
        assert list(found) == [1, 1]
        for f, im in enumerate(frames):
            want = E.latent_search(model, im, boxes[f], 0.6, None, dtype, walk, fine=True)
            r = rec[f]
            assert (r[0], r[1], r[2], r[3], r[4]) == (f, want["component"], want["level"], want["root_x"], want["root_y"]), f
            assert r[5:6].view(np.float32)[0].tobytes() == np.float32(want["score"]).tobytes()
            assert r[6] == len(want["parts"]) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want["parts"])
            assert want["found"] and want["level"] < 5
        # with the octave off no placement overlaps boxes that small by 0.6
        det.setFineOctave(False)
        rec0, found0 = det.hd.detect_latent(frames, boxes, 0.6, None)
        assert list(found0) == [0, 0]
        assert not E.latent_search(model, frames[0], boxes[0], 0.6, None, dtype, walk)["found"]
    finally:
        det.hd.close()


def _raw_and_planes(det, im, thr):
    raw = det.hd.pack_candidates(det.detect(im))
    plan = det.hd.plan(im.shape[0], im.shape[1])
    planes = {}
    for l in range(plan["nlevels"]):
        r, c = int(plan["feat_rows"][l]), int(plan["feat_cols"][l])
        if r * c:
            rootv = det.hd.get_stage(_lib.STAGE_ROOTV, 0, l, r, c)
            for comp in range(det.hd.flat.ncomponents):
                planes[(0, l, comp)] = rootv[comp]
    return raw, planes


def test_root_nms_and_top_k_with_fine_levels(frame):
    model = tiny(0.0)
    det = fine_detector(model)
    try:
        raw, planes = _raw_and_planes(det, frame, 0.0)
        same_as_ref(det.detect(frame), ref(model, frame, np.float32, tag="sel"))
        thr = np.float32(model.thresh)
        kept = {k: gridnms.grid_nms_ref(p, 2, p > thr) for k, p in planes.items()}
        want = gridnms.filter_records(raw, lambda f, l, c: kept[(f, l, c)])
        det.setRootNMS(2)
        got = det.hd.pack_candidates(det.detect(frame))
        assert 0 < len(got) < len(raw) and any(r[2] < 5 for r in got)
        assert np.array_equal(got, want)
        det.setRootNMS(0)
        for k in (1, 7, 40):
            det.setTopK(k)
            got = topk.canonical_order(det.hd.pack_candidates(det.detect(frame)))
            assert len(got) == k and np.array_equal(got, topk.top_k_records_ref(raw, k))
        det.setTopK(0)
        # suppression of the whole list
        full = det.detect(frame)
        want = list(full)
        Candidate.sort(want)
        Candidate.nonMaximaSuppression(frame.shape[:2], want, float(np.float32(0.3)))
        det.hd.set_nms(0.3)
        got = det.detect(frame)
        assert 0 < len(got) < len(full) and keys(got) == keys(want)
    finally:
        det.hd.close()


def test_depth_pruning_reads_the_fine_levels_scales(frame):
    """the rule takes a root box of width w to stand at Z = fx * width / w: at Z = 2 with fx * width = 20 only boxes about 10
    pixels wide stay -- those of the fine levels (5 cells of 2 .. 4 pixels), none of the reference's (5 cells of 4 pixels up)"""
    from partsbaseddetector_amd import depthprune
    model = tiny(0.0)
    det = fine_detector(model)
    try:
        raw = det.hd.pack_candidates(det.detect(frame))
        depth = np.full(frame.shape[:2], 2.0, np.float32)
        depth[::7, ::5] = 0            # holes
        cfg = (100.0, 0.2, 0.3)
        want = depthprune.filter_records(raw, [depth], *cfg)
        assert 0 < len(want) < len(raw) and all(r[2] < 5 for r in want) and any(r[2] < 5 for r in raw[~depthprune.keep_mask(raw, [depth], *cfg)])
        det.setDepthPrune(*cfg)
        got = det.hd.pack_candidates(det.detect(frame, depth))
        assert np.array_equal(got, want)
    finally:
        det.hd.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_marginals_of_a_fine_level(oracle, frame, dtype):
    model = tiny(0.5)
    flat = model.flatten()
    assert flat.ncomponents == 1
    det = fine_detector(model, dtype)
    try:
        det.detect(frame)
        det.hd.max_marginals(0)
        feats, _ = F.features_pyramid(flat, frame, dtype)
        plan = det.hd.plan(48, 64)
        for l in (1, 6):        # a fine level and a reference level
            H, W = int(plan["feat_rows"][l]), int(plan["feat_cols"][l])
            want = MG.max_marginals(flat, 0, oracle.responses(flat, feats[l]))
            for w, what in zip(want, (_lib.MM_VALUES, _lib.MM_DOWN, _lib.MM_PARENT_X, _lib.MM_PARENT_Y, _lib.MM_PARENT_K)):
                got = det.hd.get_marginals(l, what, H, W)
                assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), (l, what)
    finally:
        det.hd.close()


# ---- 6. plan report, refusals and state --------------------------------------------------------------------------------------
def test_refusals(frame):
    for sbin in (2, 5, 7):
        model = M.synthetic_model(seed=3, pa=[0, 1], nmix=1, sbin=sbin, interval=2, name="no-fine")
        hd = detector.Handle(model, device=0)
        try:
            with pytest.raises(PbdError) as e:
                hd.set_fine_octave(True)
            assert e.value.code == -2, sbin
            hd.set_fine_octave(False)
        finally:
            hd.close()
        det = detector.PartsBasedDetector(device=0)
        det.setFineOctave(True)
        try:
            with pytest.raises(PbdError) as e:
                det.distributeModel(model)
            assert e.value.code == -2
        finally:
            if det.hd is not None:
                det.hd.close()
    # too many levels: 118 + 30 > PBD_MAX_LEVELS, reported by the call that plans the frame
    model = M.synthetic_model(seed=3, pa=[0, 1], nmix=1, sbin=4, interval=30, thresh=1e9, name="deep")
    hd = detector.Handle(model, device=0)
    try:
        assert hd.plan(300, 300)["nlevels"] == 118
        hd.set_fine_octave(True)
        with pytest.raises(PbdError) as e:
            hd.plan(300, 300)
        assert e.value.code == -2
        with pytest.raises(PbdError) as e:
            hd.detect(synth.synthetic_frame(3, 300, 300))
        assert e.value.code == -2
        assert hd.plan(150, 150)["nlevels"] == len(F.plan(150, 150, 4, 30)[0]) == 88 + 30
        hd.set_fine_octave(False)
        assert hd.plan(300, 300)["nlevels"] == 118
    finally:
        hd.close()


def test_state(frame):
    model = tiny(0.2)
    det = detector.PartsBasedDetector(device=0, max_batch=2)
    det.distributeModel(model)
    hd = det.hd
    try:
        # in flight
        det.submit_batch([frame])
        with pytest.raises(PbdError) as e:
            hd.set_fine_octave(True)
        assert e.value.code == -5
        det.wait_batch()
        hd.set_fine_octave(True)
        cands = det.detect(frame)
        plan = hd.plan(48, 64)
        assert plan["nlevels"] == len(F.plan(48, 64, 4, 5)[0])
        r0, c0 = int(plan["feat_rows"][0]), int(plan["feat_cols"][0])
        rec = hd.pack_candidates(cands)
        # a call that changes nothing leaves the resident result; one that changes the setting drops it
        before = hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0)
        hd.set_fine_octave(True)
        assert hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0).tobytes() == before.tobytes()
        assert len(hd.examples(rec)[0]) == len(rec)
        hd.set_fine_octave(False)
        for reader in (lambda: hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0), lambda: hd.get_stage(_lib.STAGE_FEATURES, 0, 0, r0, c0),
                       lambda: hd.examples(rec), lambda: hd.part_scores(rec), lambda: hd.dp_argmin(plan["scales"])):
            with pytest.raises(PbdError) as e:
                reader()
            assert e.value.code == -5
        # a model update keeps the setting
        hd.set_fine_octave(True)
        want = keys(det.detect(frame))
        det.updateModel(hd.model_vector())
        assert keys(det.detect(frame)) == want
        same_as_ref(det.detect(frame), ref(model, frame, np.float32, tag="state"))
        # the detector keeps it across distributeModel; the pool forwards it
        det.setFineOctave(True)
        det.distributeModel(model)
        assert keys(det.detect(frame)) == want
    finally:
        det.hd.close()
    pool = detector.DetectorPool(model, n=2)
    try:
        pool.setFineOctave(True)
        assert all(keys(d.detect(frame)) == want for d in pool.dets)
    finally:
        pool.close()


# ---- 7. the planted object -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_half_size_object(oracle, dtype):
    model, im, (bx, by, side) = cases.planted(oracle)
    det = detector.PartsBasedDetector(device=0, dtype=dtype)
    det.distributeModel(model)
    try:
        assert det.detect(im) == []
        det.setFineOctave(True)
        found = det.detect(im)
        same_as_ref(found, ref(model, im, dtype, tag="planted"))
        best = max(found, key=lambda c: c.score())
        assert best.level == 0 and float(det.hd.plan(*im.shape[:2])["scales"][0]) == 2.0
        x, y, w, h = (int(v) for v in best.parts[0])
        assert abs(x - bx) <= 2 and abs(y - by) <= 2 and abs(w - side) <= 2 and abs(h - side) <= 2
    finally:
        det.hd.close()
