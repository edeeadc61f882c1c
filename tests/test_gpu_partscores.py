"""Part scores on the device (pbd_part_scores*, pbd_score_placements*) byte for byte against the numpy rule of
partsbaseddetector_amd/partscores.py walked through the oracle's maps: status, placement and the four values per part, in both
walk modes, for float and double; the score identity of the arg-max walk; mixed batches, suppression, the device forms; wide
maps, deep trees, inner parts that share filter ids, filters of several sizes, more parts than lanes; every convolution mode
against the rule fed with the mode's own resident responses; latent positives; given placements; refusals."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import partscores as PS
from partsbaseddetector_amd.detector import PbdError

from test_gpu_examples import records, shared_model

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
WALK = {"reference": _lib.WALK_REFERENCE, "argmax": _lib.WALK_ARGMAX}
SENT = -7                               # what the outputs hold before a call
TREE_PA = [0, 1, 2, 2, 1, 5, 5, 3]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


class ReadBackMaps(E.FrameMaps):
    """the yardstick's maps of frame `frame` of the resident result, its dynamic program run on the handle's own resident
    responses (pbd_get_stage: fp16 widened to float), so that no bound on an inexact convolution mode enters"""

    def __init__(self, hd, frame, flat, im, dtype=np.float32, walk="reference"):
        super().__init__(flat, im, dtype, walk)
        self.hd, self.frame = hd, frame

    def resp(self, level):
        if level not in self._resp:
            f = self.feats[level]
            self._resp[level] = self.hd.get_stage(_lib.STAGE_RESPONSES, self.frame, level, f.shape[0], f.shape[1] // E.FLEN)
        return self._resp[level]


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def check(hd, flat, maps, rec, dtype, walk):
    """status, placement and values of rec == the rule's on maps, byte for byte, what lies past a record's parts included (it
    keeps SENT); returns them"""
    got = hd.part_scores(rec, fill=SENT)
    want = PS.scores_of_records(flat, maps, rec, 0, dtype, walk, fill=SENT)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert same(got, want)
    return got


def score_bits(rec):
    return rec[:, 5].copy()


def root_bits(scores):
    return scores[:, 0, PS.MESSAGE].astype(np.float32).view(np.int32)


@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_and_shared_leaf_filters(dtype, walk):
    for model in (M.synthetic_tiny_model(thresh=-1.0), shared_model()):
        flat = model.flatten()
        hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
        try:
            hd.set_walk(WALK[walk])
            im = synth.synthetic_frame(5, 72, 96)
            rec = records(hd, [im])
            assert len(rec) > 20
            st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, dtype, walk=walk)], rec, dtype, walk)
            assert np.all(st == 3)
            got, score = root_bits(sc).view(np.float32), score_bits(rec).view(np.float32)
            if walk == "argmax":
                assert np.array_equal(root_bits(sc), score_bits(rec))     # guarantee 1: the record's score, bit for bit
            else:
                assert np.all(got <= score) and np.any(got < score)       # guarantee 2
        finally:
            hd.close()


def device_call(hd, allrec, cap, dtype, count=None, place=True, given=None, extra=4):
    """pbd_part_scores_device (given: pbd_score_placements_device) on a payload of allrec with word 0 = count, outputs of
    cap + extra records filled with SENT; returns status, place, scores as numpy"""
    import torch
    mp = (hd.stride - 8) // 4
    pay = torch.zeros(1 + max(cap, len(allrec)) * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = len(allrec) if count is None else count
    pay[1:1 + allrec.size] = torch.from_numpy(allrec.ravel()).cuda()
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_st = torch.full((cap + extra,), SENT, dtype=torch.int32, device="cuda")
    d_pl = torch.full((cap + extra, mp, 3), SENT, dtype=torch.int32, device="cuda")
    d_sc = torch.full((cap + extra, mp, 4), SENT, dtype=tdt, device="cuda")
    if given is not None:
        d_pl[:len(given)] = torch.from_numpy(np.ascontiguousarray(given, np.int32)).cuda()
    torch.cuda.synchronize()
    if given is None:
        hd.part_scores_device(pay.data_ptr(), cap, 0, d_st.data_ptr(), d_pl.data_ptr() if place else None, d_sc.data_ptr())
    else:
        hd.score_placements_device(pay.data_ptr(), cap, 0, d_pl.data_ptr(), d_st.data_ptr(), d_sc.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return d_st.cpu().numpy(), d_pl.cpu().numpy(), d_sc.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_components_mixed_batch_nms_and_device_form(dtype):
    model = M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 18)
    try:
        frames = [synth.synthetic_frame(3, 64, 80), synth.synthetic_frame(4, 96, 72), synth.synthetic_frame(6, 50, 130)]
        maps = [E.FrameMaps(flat, f, dtype) for f in frames]
        rec = records(hd, frames)
        assert len(set(rec[:, 0])) == 3 and len(set(rec[:, 1])) == 3
        sub = rec[np.random.default_rng(2).permutation(len(rec))[:300]]
        host = check(hd, flat, maps, sub, dtype, "reference")
        # the device form: the same bytes; a record outside the resident result gets -1 and nothing else
        bad = sub[:3].copy()
        bad[1, 3] = 10000
        allrec = np.concatenate([sub, bad])
        n = len(sub)
        st, pl, sc = device_call(hd, allrec, len(allrec) + 5, dtype)
        assert same((st[:n], pl[:n], sc[:n]), host)
        assert list(st[n:n + 3]) == [7, -1, 7]
        assert np.all(pl[n + 1] == SENT) and np.all(sc[n + 1] == SENT)
        assert np.all(st[n + 3:] == SENT) and np.all(pl[n + 3:] == SENT) and np.all(sc[n + 3:] == SENT)     # past the count
        # without d_place the values are the same
        st2, pl2, sc2 = device_call(hd, allrec, len(allrec) + 5, dtype, place=False)
        assert np.array_equal(st2, st) and sc2.tobytes() == sc.tobytes() and np.all(pl2 == SENT)
        # a count above the capacity is clamped to it
        st, pl, sc = device_call(hd, allrec, n - 5, dtype, count=len(allrec) + 10)
        assert same((st[:n - 5], pl[:n - 5], sc[:n - 5]), tuple(a[:n - 5] for a in host))
        assert np.all(st[n - 5:] == SENT) and np.all(pl[n - 5:] == SENT) and np.all(sc[n - 5:] == SENT)
        # a -1 payload (a suppression overflow) writes nothing
        st, pl, sc = device_call(hd, allrec, len(allrec), dtype, count=-1)
        assert np.all(st == SENT) and np.all(pl == SENT) and np.all(sc == SENT)
        # records after pbd_set_nms
        hd.set_nms(0.3)
        kept = records(hd, frames)
        assert 0 < len(kept) < len(rec)
        check(hd, flat, maps, kept, dtype, "reference")
    finally:
        hd.close()


def ragged_model():
    """three components of 7, 7 and 6 parts: the face model with the last (leaf) part of its last component taken away"""
    m = M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0)
    for tab in (m.filterid, m.biasid, m.defid, m.parentid):
        tab[2].pop()
    m.validate()
    return m


def test_values_past_a_records_parts_are_not_written():
    model = ragged_model()
    flat = model.flatten()
    hd = detector.Handle(model, device=0, max_candidates=1 << 18)
    try:
        im = synth.synthetic_frame(3, 64, 80)
        rec = records(hd, [im])
        rec = rec[np.random.default_rng(3).permutation(len(rec))[:200]]
        assert set(rec[:, 1]) == {0, 1, 2}
        st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im)], rec, np.float32, "reference")
        short = st == 6
        assert short.any() and np.array_equal(short, rec[:, 1] == 2)
        assert np.all(pl[short, 6] == SENT) and np.all(sc[short, 6] == SENT)
        dst, dpl, dsc = device_call(hd, rec, len(rec), np.float32, extra=0)
        assert same((dst, dpl, dsc), (st, pl, sc))
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wide_map_int16_planes(dtype):
    """36 x 1100 pixels: the position planes are int16 (k_ps_walk<int16_t>), and some record walks to a part beyond column 255"""
    model = M.synthetic_tiny_model(thresh=0.8)
    flat = model.flatten()
    im = synth.synthetic_frame(13, 36, 1100)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 12)
    try:
        assert int(hd.plan(36, 1100)["feat_cols"].max()) > 256
        for walk in ("reference", "argmax"):
            hd.set_walk(WALK[walk])
            rec = records(hd, [im])
            assert 100 <= len(rec) <= 600
            st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, dtype, walk=walk)], rec, dtype, walk)
            assert np.any(pl[:, 1:3, 0] >= 256)
            if walk == "argmax":
                assert np.array_equal(root_bits(sc), score_bits(rec))
    finally:
        hd.close()


def tree_model(inner_shared=False):
    m = M.synthetic_model(seed=7, pa=TREE_PA, nmix=3, linear_def=True, interval=5, thresh=-100.0)
    if inner_shared:
        m.filterid[0][4] = list(m.filterid[0][1])
        m.validate()
    return m


@pytest.mark.parametrize("inner_shared", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_three_tree_and_inner_shared_filter_ids(dtype, inner_shared):
    """8 parts, three levels of accumulation, parents with two children.  With inner parts that share filter ids (the
    sequential schedule) the values are still the rule's; the score identity is not asserted there (guarantee 3)"""
    model = tree_model(inner_shared)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18)
    try:
        im = synth.synthetic_frame(3, 64, 80)
        for walk in ("reference", "argmax"):
            hd.set_walk(WALK[walk])
            rec = records(hd, [im])
            rec = rec[np.random.default_rng(4).permutation(len(rec))[:200]]
            assert len(rec) == 200
            st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, dtype, walk=walk)], rec, dtype, walk)
            if walk == "argmax" and not inner_shared:
                assert np.array_equal(root_bits(sc), score_bits(rec))
    finally:
        hd.close()


def test_filters_of_several_sizes():
    model = M.synthetic_model(seed=3, pa=[0, 1, 1], nmix=2, ksize=[3, 5, 7], linear_def=True, interval=5, thresh=-1.0)
    flat = model.flatten()
    assert len(set(int(k) for k in flat.filter_ksize)) == 3
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        hd.set_walk(_lib.WALK_ARGMAX)
        im = synth.synthetic_frame(5, 72, 96)
        rec = records(hd, [im])
        assert len(rec) > 20
        st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, walk="argmax")], rec[:300], np.float32, "argmax")
        assert np.array_equal(root_bits(sc), score_bits(rec[:300]))
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_more_parts_than_lanes(dtype):
    """70 parts (a root with 40 children, the first of which has 29): lanes stride over the parts (parts 64..69 are a lane's
    second) and one parent accumulates 40 messages"""
    model = M.synthetic_model(seed=9, pa=[0] + [1] * 40 + [2] * 29, nmix=1, linear_def=True, interval=2, thresh=-100.0)
    flat = model.flatten()
    assert flat.max_parts == 70
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
    try:
        hd.set_walk(_lib.WALK_ARGMAX)
        im = synth.synthetic_frame(8, 48, 56)
        rec = records(hd, [im])
        rec = rec[np.random.default_rng(5).permutation(len(rec))[:60]]
        assert len(rec) >= 30
        st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, dtype, walk="argmax")], rec, dtype, "argmax")
        assert np.all(st == 70)
        assert np.array_equal(root_bits(sc), score_bits(rec))
    finally:
        hd.close()


@pytest.mark.parametrize("mode,dtype", [(_lib.CONV_FMA, np.float32), (_lib.CONV_MFMA, np.float32), (_lib.CONV_MFMA_F16, np.float32),
                                        (_lib.CONV_MFMA_ANY, np.float32), (_lib.CONV_MFMA_F16_ANY, np.float32),
                                        (_lib.CONV_MFMA_F64, np.float64)])
def test_every_convolution_mode_on_its_own_resident_responses(mode, dtype):
    """appearance is the resident response at the cell (fp16 residency widened), and all four values are the rule's when the
    rule's dynamic program runs on the responses read back from the handle"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, conv_mode=mode, real_type=REAL[dtype], max_candidates=1 << 16)
    try:
        hd.set_walk(_lib.WALK_ARGMAX)
        im = synth.synthetic_frame(5, 72, 96)
        rec = records(hd, [im])
        assert len(rec) > 20
        fm = ReadBackMaps(hd, 0, flat, im, dtype, walk="argmax")
        st, pl, sc = check(hd, flat, [fm], rec, dtype, "argmax")
        for i, r in enumerate(rec):
            resp = fm.resp(int(r[2]))
            for p in range(st[i]):
                x, y, m = pl[i, p]
                f = int(flat.filterid[int(flat.mix_offset[p]) + m])
                assert sc[i, p, PS.APPEARANCE].tobytes() == resp[f, y, x].tobytes()
        assert np.array_equal(root_bits(sc), score_bits(rec))
    finally:
        hd.close()


@pytest.mark.parametrize("walk", ["reference", "argmax"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_after_detect_latent(dtype, walk):
    """the resident result of pbd_detect_latent: one response plane per (component, part, mixture), masked"""
    from oracle import oracle
    from test_gpu_walk import oracle_boxes
    model = M.synthetic_tiny_model(thresh=-100.0)
    flat = model.flatten()
    uflat = E.unique_model(model).flatten()
    frames = [synth.synthetic_frame(s, 72, 96) for s in (5, 7, 9, 11)]
    boxes = [oracle_boxes(flat, im) for im in frames]
    overlap = 0.6
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 16)
    try:
        hd.set_walk(WALK[walk])
        rec, found = hd.detect_latent(frames, boxes, overlap)
        assert found.any()
        keep = np.nonzero(found)[0]
        st, pl, sc = hd.part_scores(rec[keep], fill=SENT)
        for k, f in enumerate(keep):
            want = E.latent_search(model, frames[f], boxes[f], overlap, None, dtype, walk=walk)
            feats, scales = oracle.features_pyramid(uflat, frames[f], dtype)
            lvl, c = want["level"], want["component"]
            resp = E.mask_responses(uflat, oracle.responses(uflat, feats[lvl]), scales[lvl], boxes[f], overlap, None, dtype)
            assert st[k] == 3 and np.array_equal(pl[k], np.asarray(want["placement"], np.int32))
            assert sc[k].tobytes() == PS.part_scores(uflat, resp, c, want["placement"], dtype).tobytes(), f
            if walk == "argmax":
                assert root_bits(sc[k:k + 1])[0] == rec[f, 5]
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score_placements(dtype):
    model = tree_model()
    flat = model.flatten()
    parent = [int(p) for p in flat.parentid[:8]]
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18)
    try:
        im = synth.synthetic_frame(3, 64, 80)
        rec = records(hd, [im])
        rec = rec[np.random.default_rng(6).permutation(len(rec))[:100]]
        maps = [E.FrameMaps(flat, im, dtype)]
        st, pl, sc = hd.part_scores(rec, fill=SENT)
        # the walk's own placements: the bytes of part_scores, whatever the records' root cells say
        moved = rec.copy()
        moved[:, 3:5] = 10000
        st2, sc2 = hd.score_placements(moved, pl, fill=SENT)
        assert np.array_equal(st2, st) and sc2.tobytes() == sc.tobytes()
        # one leaf (part 7, under 2, 1, 0) moved by one cell: its appearance and message, its ancestors' total and message
        plan = hd.plan(64, 80)
        new = pl.copy()
        for i, r in enumerate(rec):
            W = int(plan["feat_cols"][int(r[2])])
            new[i, 7, 0] += 1 if new[i, 7, 0] + 1 < W else -1
        st3, sc3 = hd.score_placements(rec, new, fill=SENT)
        want = PS.scores_of_records(flat, maps, rec, 0, dtype, place=new, fill=SENT)
        assert np.array_equal(st3, want[0]) and sc3.tobytes() == want[2].tobytes()
        diff = sc3.view(np.uint32 if dtype == np.float32 else np.uint64) != sc.view(np.uint32 if dtype == np.float32 else np.uint64)
        may = np.zeros((8, 4), bool)
        may[7, [PS.APPEARANCE, PS.MESSAGE, PS.TOTAL]] = True
        for a in (2, 1, 0):
            may[a, [PS.MESSAGE, PS.TOTAL]] = True
        assert parent[7] == 2 and parent[2] == 1 and parent[1] == 0
        assert not np.any(diff & ~may[None]) and np.any(diff[:, 7, PS.APPEARANCE]) and np.any(diff[:, 0, PS.MESSAGE])
        # a cell outside the map, a mixture outside the part's range: -1 for that record only
        bad = pl.copy()
        bad[3, 5, 0] = 10000
        bad[10, 2, 1] = -1
        bad[20, 6, 2] = 3
        bad[30, 0, 2] = -1
        st4, sc4 = hd.score_placements(rec, bad, fill=SENT)
        hit = np.zeros(len(rec), bool)
        hit[[3, 10, 20, 30]] = True
        assert np.all(st4[hit] == -1) and np.all(sc4[hit] == SENT)
        assert np.array_equal(st4[~hit], st[~hit]) and sc4[~hit].tobytes() == sc[~hit].tobytes()
        # the device form
        dst, _, dsc = device_call(hd, rec, len(rec), dtype, given=bad, extra=0)
        assert np.array_equal(dst, st4) and dsc.tobytes() == sc4.tobytes()
    finally:
        hd.close()


def resident_bytes(hd, im):
    p = hd.plan(*im.shape[:2])
    out = []
    for lvl in range(p["nlevels"]):
        rows, cols = int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl])
        if rows * cols:
            out += [hd.get_stage(s, 0, lvl, rows, cols).tobytes() for s in (_lib.STAGE_RESPONSES, _lib.STAGE_ROOTV, _lib.STAGE_ROOTI)]
    return out


def test_refusals_leave_everything_as_it_was():
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        rec0 = np.zeros((1, hd.stride), np.int32)
        pl0 = np.zeros((1, 3, 3), np.int32)
        for call in (lambda: hd.part_scores(rec0), lambda: hd.score_placements(rec0, pl0),
                     lambda: device_call(hd, rec0, 1, np.float32), lambda: device_call(hd, rec0, 1, np.float32, given=pl0)):
            with pytest.raises(PbdError) as e:
                call()
            assert e.value.code == -5             # no resident result yet
        im = synth.synthetic_frame(5, 72, 96)
        rec = records(hd, [im])
        before = resident_bytes(hd, im)
        ex_before = hd.examples(rec)
        good = hd.part_scores(rec, fill=SENT)
        for field, value in ((0, 1), (2, 99), (1, 5), (3, -1), (4, 10000)):
            bad = rec[:4].copy()
            bad[2, field] = value
            with pytest.raises(PbdError) as e:
                hd.part_scores(bad)
            assert e.value.code == -1 and "record 2" in str(e.value)
            if field < 3:                         # given placements ignore the record's root cell
                with pytest.raises(PbdError) as e:
                    hd.score_placements(bad, good[1][:4])
                assert e.value.code == -1 and "record 2" in str(e.value)
        assert hd.part_scores(rec[:0])[0].shape == (0,)
        # while a batch is in flight
        f = np.ascontiguousarray(im)
        hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 1, _lib.ptr_array([f]), f.shape[0], f.shape[1], f.shape[2],
                                                f.shape[1] * f.shape[2]))
        try:
            for call in (lambda: hd.part_scores(rec), lambda: hd.score_placements(rec, good[1]),
                         lambda: device_call(hd, rec, len(rec), np.float32)):
                with pytest.raises(PbdError) as e:
                    call()
                assert e.value.code == -5
        finally:
            buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
            n = C.c_int()
            hd.check(hd.lib.pbd_detect_batch_wait(hd.h, buf.ctypes.data, hd.max_candidates, C.byref(n)))
        assert np.array_equal(buf[:n.value * hd.stride].reshape(-1, hd.stride), rec)
        # nothing above changed the resident result, the calls' own results, a later detect call or examples()
        assert resident_bytes(hd, im) == before
        assert same(hd.part_scores(rec, fill=SENT), good)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(hd.examples(rec), ex_before))
        assert np.array_equal(records(hd, [im]), rec)
        # after pbd_dp_min, after a model update, after pbd_conv_set_filters: no resident result
        from oracle import oracle
        feats, _ = oracle.features_pyramid(flat, im, np.float32)
        detector.DynamicProgram(hd).min([oracle.responses(flat, feats[0])])
        with pytest.raises(PbdError) as e:
            hd.part_scores(rec[:1])
        assert e.value.code == -5
        assert np.array_equal(records(hd, [im]), rec) and same(hd.part_scores(rec, fill=SENT), good)
        hd.set_model_vector(hd.model_vector())
        with pytest.raises(PbdError) as e:
            hd.part_scores(rec[:1])
        assert e.value.code == -5
        assert np.array_equal(records(hd, [im]), rec) and same(hd.part_scores(rec, fill=SENT), good)
        filt = [np.ascontiguousarray(w, np.float32) for w in model.filtersw]
        ks = np.array(flat.filter_ksize, np.int32)
        hd.check(hd.lib.pbd_conv_set_filters(hd.h, len(filt), _lib.ptr_array(filt), _lib.ptr(ks, C.c_int)))
        for call in (lambda: hd.part_scores(rec[:1]), lambda: hd.score_placements(rec[:1], good[1][:1])):
            with pytest.raises(PbdError) as e:
                call()
            assert e.value.code == -5
    finally:
        hd.close()


def test_a_model_update_reaches_the_part_scores():
    """the deformation and bias values are those of the handle's current model"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        im = synth.synthetic_frame(5, 72, 96)
        records(hd, [im])
        w = hd.model_vector()
        nb, nd = len(model.biasw), len(model.defw)
        w[:nb] += 0.125
        w[nb:nb + 4 * nd] *= 1.5
        hd.set_model_vector(w)
        new = hd.current_model()
        hd.set_walk(_lib.WALK_ARGMAX)
        rec = records(hd, [im])
        assert len(rec) > 20
        flat = new.flatten()
        st, pl, sc = check(hd, flat, [E.FrameMaps(flat, im, walk="argmax")], rec, np.float32, "argmax")
        assert np.array_equal(root_bits(sc), score_bits(rec))
    finally:
        hd.close()


def test_python_mirror_fills_confidences_and_mixtures():
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    det = detector.PartsBasedDetector(device=0)
    det.distributeModel(model)
    im = synth.synthetic_frame(5, 72, 96)
    cands = det.detect(im)
    scores0 = [c.score() for c in cands]
    assert all(len(c.confidence) == 3 and not c.confidence[1:].any() and c.mixtures is None for c in cands)
    place, scores = det.partScores(cands)
    fm = E.FrameMaps(flat, im)
    for i, c in enumerate(cands):
        pl = fm.placement(c.level, c.component, c.root[0], c.root[1])
        want = PS.part_scores(flat, fm.resp(c.level), c.component, pl)
        assert scores[i].tobytes() == want.tobytes() and np.array_equal(place[i], np.asarray(pl, np.int32))
        assert c.score() == scores0[i] and c.confidence.dtype == np.float32 and len(c.confidence) == 3
        assert c.confidence[1:].tobytes() == want[1:, PS.APPEARANCE].tobytes()
        assert list(c.mixtures) == [m for _, _, m in pl]
    # records in, and the placements given back
    rec = det.hd.pack_candidates(cands)
    place2, scores2 = det.partScores(rec)
    assert np.array_equal(place2, place) and scores2.tobytes() == scores.tobytes()
    st, sc = det.scorePlacements(cands, place)
    assert np.all(st == 3) and sc.tobytes() == scores.tobytes()
    det.hd.close()
