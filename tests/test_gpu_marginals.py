"""Max-marginals on the device (pbd_max_marginals, pbd_get_marginals, pbd_marginal_poses*) byte for byte against the numpy rule of
partsbaseddetector_amd/marginals.py: every plane of every level of the cases of marginal_cases.py in both value sets, for float and
double; the decoded poses word for word, host and device form; the resident detection result untouched; a frame of a batch on its
own resident responses; a model update; nBestPoses; every refusal."""
import numpy as np
import pytest

import marginal_cases as MC
from partsbaseddetector_amd import _lib, detector, gridnms, synth, topk
from partsbaseddetector_amd import marginals as MG
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {"float32": _lib.REAL_F32, "float64": _lib.REAL_F64}
DTYPES = ("float32", "float64")
SENT = -7                               # what the outputs hold before a call
WHAT = (("mm", _lib.MM_VALUES), ("down", _lib.MM_DOWN), ("Jx", _lib.MM_PARENT_X), ("Jy", _lib.MM_PARENT_Y), ("Jk", _lib.MM_PARENT_K))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def resident(name, levels, values, dtype):
    """a handle with the case's dynamic program resident (pbd_dp_min on the case's responses) and what dp_min returned"""
    hd = detector.Handle(MC.model(name, values), device=0, max_candidates=1 << 12, real_type=REAL[dtype])
    out = detector.DynamicProgram(hd).min(MC.responses(name, levels, values, dtype))
    return hd, out


def check_planes(hd, shapes, want_of):
    for key, what in WHAT:
        want = want_of(key)
        for l, (H, W) in enumerate(shapes):
            got = hd.get_marginals(l, what, H, W)
            assert got.dtype == want[l].dtype and got.shape == want[l].shape, (key, l)
            assert got.tobytes() == want[l].tobytes(), (key, l, np.argwhere(got != want[l])[:4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("values", MC.VALUES)
@pytest.mark.parametrize("name,levels", MC.CASES)
def test_every_plane_equals_the_rule(name, levels, values, dtype):
    hd, _ = resident(name, levels, values, dtype)
    try:
        hd.max_marginals(0)
        check_planes(hd, MC.LEVEL_SETS[levels], lambda key: MC.merged(name, levels, values, dtype, key))
    finally:
        hd.close()


def device_poses(hd, seeds, scales, frame_offset, want_place=True):
    import torch
    n = len(seeds)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.int32)).cuda()
    d_rec = torch.full((n, hd.stride), SENT, dtype=torch.int32, device="cuda")
    d_place = torch.full((n, hd.max_parts, 3), SENT, dtype=torch.int32, device="cuda")
    d_status = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.marginal_poses_device(n, d_seeds.data_ptr(), scales, frame_offset, d_rec.data_ptr(), d_place.data_ptr() if want_place else None,
                             d_status.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return d_status.cpu().numpy(), d_rec.cpu().numpy(), d_place.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("values", MC.VALUES)
@pytest.mark.parametrize("name,levels", [("chain", "A"), ("star", "A"), ("tree", "B"), ("two", "A"), ("slices", "B")])
def test_poses_equal_the_rules_decode(name, levels, values, dtype):
    hd, _ = resident(name, levels, values, dtype)
    try:
        hd.max_marginals(0)
        seeds = MC.seeds_of(name, levels, values, dtype)
        sc = MC.scales(levels)
        want = MC.decode_all(name, levels, values, dtype, seeds, frame_offset=5, fill=SENT)
        assert (want[0] > 0).sum() >= 6 and (want[0] == -1).sum() == 9
        got = hd.marginal_poses(seeds, sc, 5, fill=SENT)
        for g, w, what in zip(got, want, ("status", "records", "place")):
            assert np.array_equal(g, w), (what, np.argwhere(g != w)[:4])
        dev = device_poses(hd, seeds, sc, 5)
        # the device form writes nothing of a bad seed either; a pose's record is written whole (the boxes past its parts are not)
        for g, w, what in zip(dev, want, ("status", "records", "place")):
            assert np.array_equal(g, w), (what, np.argwhere(g != w)[:4])
        dev2 = device_poses(hd, seeds, sc, 5, want_place=False)
        assert np.array_equal(dev2[0], want[0]) and np.array_equal(dev2[1], want[1])
        with pytest.raises(PbdError) as e:            # a pbd_dp_min result has no scales of its own
            hd.marginal_poses(seeds[:1], None)
        assert e.value.code == -1
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_resident_detection_result_is_untouched(dtype):
    name, levels = "tree", "B"
    hd, before = resident(name, levels, "dense", dtype)
    try:
        dp = detector.DynamicProgram(hd)
        sc = MC.scales(levels)
        shapes = MC.LEVEL_SETS[levels]
        cand0 = hd.pack_candidates(dp.argmin(sc))
        rootv0 = [hd.get_stage(_lib.STAGE_ROOTV, 0, l, H, W).tobytes() for l, (H, W) in enumerate(shapes)]
        rooti0 = [hd.get_stage(_lib.STAGE_ROOTI, 0, l, H, W).tobytes() for l, (H, W) in enumerate(shapes)]
        assert len(cand0) > 10
        hd.max_marginals(0)
        hd.marginal_poses(MC.seeds_of(name, levels, "dense", dtype), sc)
        assert np.array_equal(hd.pack_candidates(dp.argmin(sc)), cand0)
        assert rootv0 == [hd.get_stage(_lib.STAGE_ROOTV, 0, l, H, W).tobytes() for l, (H, W) in enumerate(shapes)]
        assert rooti0 == [hd.get_stage(_lib.STAGE_ROOTI, 0, l, H, W).tobytes() for l, (H, W) in enumerate(shapes)]
        # the marginals survive the reads, and a second call gives the same planes
        hd.max_marginals(0)
        check_planes(hd, shapes, lambda key: MC.merged(name, levels, "dense", dtype, key))
        # reduceMax over the root's types is the root score, read from the device
        flat = hd.flat
        for l, (H, W) in enumerate(shapes):
            mm = hd.get_marginals(l, _lib.MM_VALUES, H, W)
            v, i = MG.reduce_max([mm[g] for g in MC.part_planes(flat, 0, 0)])
            assert v.tobytes() == before[3][l][0].tobytes() and np.array_equal(i, before[4][l][0])
    finally:
        hd.close()


def merged_rule(flat, resp):
    """marginals.max_marginals of every component on one level's responses, merged as pbd_get_marginals returns them"""
    out = None
    for c in range(flat.ncomponents):
        r = MG.max_marginals(flat, c, resp)
        if out is None:
            out = [np.array(a, copy=True) for a in r]
            continue
        g0, g1 = int(flat.mix_offset[flat.part_offset[c]]), int(flat.mix_offset[flat.part_offset[c + 1]])
        for a, b in zip(out, r):
            a[g0:g1] = b[g0:g1]
    return dict(zip(("mm", "down", "Jx", "Jy", "Jk"), out))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_frame_one_of_a_batch_on_its_own_responses(dtype):
    """the synthetic person model on two small frames: frame 1's planes equal the rule run on frame 1's resident responses (three
    of its levels: the rule takes a second per level for this model)"""
    model = M.synthetic_person_model(thresh=0.0)
    det = detector.PartsBasedDetector(device=0, max_batch=2, max_candidates=1 << 16, dtype=dtype)
    det.distributeModel(model)
    try:
        frames = [synth.synthetic_frame(11, 40, 56), synth.synthetic_frame(12, 40, 56)]
        det.detect_batch(frames)
        hd, flat = det.hd, det.hd.flat
        shapes = hd.level_shapes
        mm = det.maxMarginals(frame=1)
        assert len(mm) == len(shapes) >= 6
        for l in (0, len(shapes) // 2, len(shapes) - 1):
            H, W = shapes[l]
            resp = hd.get_stage(_lib.STAGE_RESPONSES, 1, l, H, W)
            want = merged_rule(flat, resp)
            assert mm[l].tobytes() == want["mm"].tobytes(), l
            for key, what in WHAT[1:]:
                assert hd.get_marginals(l, what, H, W).tobytes() == want[key].tobytes(), (key, l)
        # a root seed decodes to the detection the arg-max walk reports there, scored by pbd_score_placements bit for bit
        l = len(shapes) // 2
        H, W = shapes[l]
        pl = MC.part_planes(flat, 0, 0)
        blk = mm[l][pl[0]:pl[-1] + 1]
        t, y, x = np.unravel_index(int(np.argmax(blk)), blk.shape)
        status, rec, place = hd.marginal_poses(np.array([[l, 0, 0, -1, x, y]], np.int32), None, 0)
        assert status[0] == flat.max_parts and rec[0, 0] == 1 and tuple(rec[0, 3:5]) == (x, y) and rec[0, 7] == t
        st, scores = hd.score_placements(rec, place)
        assert st[0] == flat.max_parts
        assert np.float32(scores[0, 0, 1]).tobytes() == rec[0, 5:6].tobytes()
        with pytest.raises(PbdError) as e:
            det.hd.max_marginals(2)
        assert e.value.code == -1
    finally:
        det.hd.close()


def test_after_a_model_update_the_marginals_are_the_new_models():
    model = M.synthetic_tiny_model(thresh=-1.0)
    im = synth.synthetic_frame(5, 48, 64)
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        det.detect(im)
        old = det.maxMarginals()
        w = model.to_vector(np.float32)
        rng = np.random.default_rng(3)
        w2 = (w * (1.0 + 0.2 * rng.standard_normal(w.size))).astype(np.float32)
        nb = len(model.biasw)
        w2[nb:nb + 4 * len(model.defw)] = np.abs(w2[nb:nb + 4 * len(model.defw)]) + 0.001       # the quadratic terms stay positive
        det.updateModel(w2)
        with pytest.raises(PbdError) as e:            # the update left no resident result
            det.hd.max_marginals(0)
        assert e.value.code == -5
        det.detect(im)
        got = det.maxMarginals()
        fresh = detector.PartsBasedDetector(device=0, max_candidates=1 << 16)
        fresh.distributeModel(model.from_vector(w2))
        try:
            fresh.detect(im)
            want = fresh.maxMarginals()
            assert len(got) == len(want) >= 3
            assert all(g.tobytes() == w_.tobytes() for g, w_ in zip(got, want))
            assert any(g.tobytes() != o.tobytes() for g, o in zip(got, old))
            for l, (H, W) in enumerate(det.hd.level_shapes):
                for _, what in WHAT[1:]:
                    assert det.hd.get_marginals(l, what, H, W).tobytes() == fresh.hd.get_marginals(l, what, H, W).tobytes()
        finally:
            fresh.hd.close()
    finally:
        det.hd.close()


def expect(code, call):
    with pytest.raises(PbdError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refused_without_a_resident_result_and_for_a_bad_frame():
    model = M.synthetic_tiny_model(thresh=-1.0)
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 16)
    det.distributeModel(model)
    hd = det.hd
    try:
        seeds = np.zeros((1, 6), np.int32)
        expect(-5, lambda: hd.max_marginals(0))
        expect(-5, lambda: hd.get_marginals(0, _lib.MM_VALUES, 4, 4))
        expect(-5, lambda: hd.marginals_device(0))
        expect(-5, lambda: hd.marginal_poses(seeds, np.ones(1, np.float32)))
        expect(-5, lambda: det.maxMarginals())
        det.detect(synth.synthetic_frame(5, 48, 64))
        expect(-1, lambda: hd.max_marginals(1))
        expect(-1, lambda: hd.max_marginals(-1))
        expect(-5, lambda: hd.get_marginals(0, _lib.MM_VALUES, 4, 4))       # a refused call holds nothing
        hd.max_marginals(0)
        H, W = hd.level_shapes[0]
        expect(-1, lambda: hd.get_marginals(len(hd.level_shapes), _lib.MM_VALUES, H, W))
        expect(-1, lambda: hd.get_marginals(0, 9, H, W))
        assert hd.lib.pbd_get_marginals(hd.h, 0, _lib.MM_VALUES, np.zeros(4, np.float32).ctypes.data, 16) == -1
        assert hd.marginal_poses(seeds[:0], None)[0].shape == (0,)
        # the next detect call drops them
        det.detect(synth.synthetic_frame(5, 48, 64))
        expect(-5, lambda: hd.get_marginals(0, _lib.MM_VALUES, H, W))
        expect(-5, lambda: hd.marginal_poses(seeds, None))
    finally:
        hd.close()


def test_refused_after_a_model_update():
    model = M.synthetic_tiny_model(thresh=-1.0)
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        det.detect(synth.synthetic_frame(5, 48, 64))
        det.hd.max_marginals(0)
        det.hd.set_model_vector(det.hd.model_vector())
        H, W = det.hd.level_shapes[0]
        expect(-5, lambda: det.hd.max_marginals(0))
        expect(-5, lambda: det.hd.get_marginals(0, _lib.MM_VALUES, H, W))
        expect(-5, lambda: det.hd.marginal_poses(np.zeros((1, 6), np.int32), None))
    finally:
        det.hd.close()


def test_refused_on_a_latent_result():
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        im = synth.synthetic_frame(5, 72, 96)
        hd.detect_latent([im], [[(8, 8, 40, 40)] * 3], 0.1)
        expect(-5, lambda: hd.max_marginals(0))
    finally:
        hd.close()


def test_refused_on_the_sequential_schedule():
    model = M.synthetic_tiny_model(thresh=-1.0)
    model.filterid[0][2] = list(model.filterid[0][1])         # two parts of the component share their filter ids
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        rng = np.random.default_rng(1)
        detector.DynamicProgram(hd).min([rng.standard_normal((hd.flat.nfilters, 5, 6)).astype(np.float32)])
        expect(-2, lambda: hd.max_marginals(0))
    finally:
        hd.close()


@pytest.mark.parametrize("mode", [_lib.CONV_MFMA_F16, _lib.CONV_MFMA_F16_ANY])
def test_refused_with_fp16_resident_responses(mode):
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16, conv_mode=mode)
    try:
        rng = np.random.default_rng(1)
        detector.DynamicProgram(hd).min([rng.standard_normal((hd.flat.nfilters, 5, 6)).astype(np.float32)])
        expect(-2, lambda: hd.max_marginals(0))
    finally:
        hd.close()


def test_refused_on_a_mixed_size_result():
    model = M.synthetic_tiny_model(thresh=-1.0)
    det = detector.PartsBasedDetector(device=0, max_batch=2, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        det.detect_frames([synth.synthetic_frame(5, 48, 64), synth.synthetic_frame(6, 40, 72)])
        expect(-2, lambda: det.hd.max_marginals(0))
    finally:
        det.hd.close()


def test_refused_on_a_level_sharded_handle():
    model = M.synthetic_tiny_model(thresh=-1.0)
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        det.hd.set_level_shard(0, 2)
        det.detect(synth.synthetic_frame(5, 48, 64))
        expect(-2, lambda: det.hd.max_marginals(0))
    finally:
        det.hd.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_best_poses_are_the_rules_in_order(dtype):
    name, levels, values = "tree", "A", "dense"
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 12, dtype=np.dtype(dtype))
    det.distributeModel(MC.model(name, values))
    try:
        det.dp_.min(MC.responses(name, levels, values, dtype))
        flat = det.hd.flat
        sc = MC.scales(levels)
        shapes = MC.LEVEL_SETS[levels]
        part, k, sz = 4, 7, 2
        pl = MC.part_planes(flat, 0, part)
        red = [a[pl[0]:pl[-1] + 1].max(0) for a in MC.merged(name, levels, values, dtype, "mm")]
        grid = np.concatenate([gridnms.grid_nms_ref(r, sz).ravel() for r in red])
        keep = topk.top_k_cells_ref(np.concatenate([r.ravel() for r in red]), k, grid)
        off = np.concatenate([[0], np.cumsum([H * W for H, W in shapes])])
        seeds = []
        for i in np.flatnonzero(keep):
            l = int(np.searchsorted(off, i, side="right")) - 1
            y, x = divmod(int(i - off[l]), shapes[l][1])
            seeds.append((l, 0, part, -1, x, y))
        assert len(seeds) == k
        status, rec, place = MC.decode_all(name, levels, values, dtype, np.asarray(seeds, np.int32))
        order = np.argsort(-rec[:, 5].copy().view(np.float32), kind="stable")
        got = det.nBestPoses(part, k, sz, scales=sc)
        assert len(got) == k
        assert np.array_equal(det.hd.pack_candidates(got)[:, :7], rec[order][:, :7])
        assert np.array_equal(det.hd.pack_candidates(got)[:, 8:], rec[order][:, 8:])
        for c, i in zip(got, order):
            assert np.array_equal(c.place, place[i, :status[i], :2]) and np.array_equal(c.mixtures, place[i, :status[i], 2])
        # the views are the resident block
        views = det.maxMarginals(device=True)
        for v, w in zip(views, MC.merged(name, levels, values, dtype, "mm")):
            assert v.cpu().numpy().tobytes() == w.tobytes()
    finally:
        det.hd.close()
