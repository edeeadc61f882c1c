"""The arg-max walk on the device (pbd_set_walk, PBD_WALK_ARGMAX) bit for bit against the numpy yardstick (examples.raw_maps and
walk(argmax=True), pinned on the oracle by tests/test_walk_cpu.py) in PBD_CONV_EXACT for float and double: the records' part
boxes, the example headers and values, and the score identity w . x == score for EVERY example; switching back; pbd_set_nms in
arg-max mode; latent positives in arg-max mode; refusals."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

from test_gpu_examples import records, shared_model
from test_gpu_nms import mirror

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def yardstick_parts(flat, fm, r, dtype):
    """the (nparts, 4) x, y, w, h of record r walked through fm in fm's mode"""
    lvl, c = int(r[2]), int(r[1])
    pl = fm.placement(lvl, c, int(r[3]), int(r[4]))
    out = []
    for p, (x, y, m) in enumerate(pl):
        gm = int(flat.mix_offset[flat.part_offset[c] + p]) + m
        x1, y1, x2, y2 = E.part_rects(x, y, int(flat.filter_ksize[flat.filterid[gm]]), fm.scales[lvl], dtype)
        out.append((int(x1), int(y1), int(x2 - x1), int(y2 - y1)))
    return np.asarray(out, np.int32)


def check_argmax(hd, flat, frames, rec, dtype, maps=None):
    """rec (records of a detect call in arg-max mode): part boxes, example headers and values == the yardstick's, bit for bit;
    |w . x - score| within the rounding bound plus half an ulp of the float score, for every example"""
    maps = [E.FrameMaps(flat, f, dtype, walk="argmax") for f in frames] if maps is None else maps
    for i, r in enumerate(rec):
        want = yardstick_parts(flat, maps[int(r[0])], r, dtype)
        assert r[6] == len(want) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want), i
    hdr, vals = hd.examples(rec)
    want_h, want_v = E.examples_of_records(flat, maps, rec, 0, dtype)
    assert np.array_equal(hdr, want_h)
    for i in range(len(rec)):
        n = int(hdr[i, 3])
        assert vals[i, :n].tobytes() == want_v[i, :n].tobytes(), i
    w = hd.model_vector()
    got = E.dot(hdr, vals, w)
    bound = E.rounding_bound(flat, hdr, vals, w, dtype)
    score = rec[:, 5].view(np.float32).astype(np.float64)
    bad = np.nonzero(np.abs(got - score) > bound + np.abs(score) * 2.0 ** -24)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], score[bad[:5]], bound[bad[:5]])
    return maps


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_and_shared_filters_bit_for_bit(dtype):
    for model in (M.synthetic_tiny_model(thresh=-1.0), shared_model()):
        flat = model.flatten()
        hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
        try:
            im = synth.synthetic_frame(5, 72, 96)
            ref = records(hd, [im])
            hd.set_walk(_lib.WALK_ARGMAX)
            rec = records(hd, [im])
            assert len(rec) > 20
            # the same roots and scores; the part boxes differ at some record
            assert np.array_equal(rec[:, :8], ref[:, :8]) and not np.array_equal(rec, ref)
            check_argmax(hd, flat, [im], rec, dtype)
        finally:
            hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_components_mixed_batch(dtype):
    model = M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 18)
    try:
        hd.set_walk(_lib.WALK_ARGMAX)
        frames = [synth.synthetic_frame(3, 64, 80), synth.synthetic_frame(4, 96, 72), synth.synthetic_frame(6, 50, 130)]
        rec = records(hd, frames)
        assert len(set(rec[:, 0])) == 3 and len(set(rec[:, 1])) == 3
        sub = rec[np.random.default_rng(2).permutation(len(rec))[:300]]
        check_argmax(hd, flat, frames, sub, dtype)
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wide_map_int16_planes(dtype):
    """36 x 1100 pixels: the position planes are int16 (k_argmin_walk / k_ex_walk <R, int16_t>), and some record walks to a
    part beyond column 255"""
    model = M.synthetic_tiny_model(thresh=0.8)
    flat = model.flatten()
    im = synth.synthetic_frame(13, 36, 1100)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 12)
    try:
        assert int(hd.plan(36, 1100)["feat_cols"].max()) > 256
        hd.set_walk(_lib.WALK_ARGMAX)
        rec = records(hd, [im])
        assert 100 <= len(rec) <= 600
        maps = check_argmax(hd, flat, [im], rec, dtype)
        walked = [maps[0].placement(int(r[2]), int(r[1]), int(r[3]), int(r[4])) for r in rec]
        assert any(x >= 256 for pl in walked for (x, _, _) in pl[1:])
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_person_model_150_seeded_records(dtype):
    """26 parts: in reference mode no sampled record satisfies the identity; in arg-max mode every one does"""
    model = M.synthetic_person_model(thresh=-100.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18)
    try:
        hd.set_walk(_lib.WALK_ARGMAX)
        im = synth.synthetic_frame(2, 120, 160)
        rec = records(hd, [im])
        assert len(rec) > 100
        sub = rec[np.random.default_rng(1).permutation(len(rec))[:150]]
        check_argmax(hd, flat, [im], sub, dtype)
    finally:
        hd.close()


def test_switching_back_rewalks_the_resident_result():
    """pbd_argmin_device_out re-walks the resident result in the mode current at the call; the result is not dropped"""
    import torch
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        im = synth.synthetic_frame(5, 72, 96)
        ref = records(hd, [im])
        cap = len(ref) + 3
        pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")

        def reemit():
            pay.zero_()
            hd.check(hd.lib.pbd_argmin_device_out(hd.h, 0, pay.data_ptr(), cap))
            hd.check(hd.lib.pbd_synchronize(hd.h))
            return pay.cpu().numpy().tobytes()
        before = reemit()
        assert np.frombuffer(before, np.int32)[0] == len(ref)
        assert np.array_equal(np.frombuffer(before, np.int32)[1:1 + ref.size].reshape(ref.shape), ref)
        hd.set_walk(_lib.WALK_ARGMAX)
        arg = np.frombuffer(reemit(), np.int32)
        assert arg[0] == len(ref) and arg.tobytes() != before
        check_argmax(hd, model.flatten(), [im], arg[1:1 + ref.size].reshape(ref.shape), np.float32)
        hd.set_walk(_lib.WALK_REFERENCE)
        assert reemit() == before
        hdr, vals = hd.examples(ref)
        want_h, want_v = E.examples_of_records(model.flatten(), [E.FrameMaps(model.flatten(), im)], ref)
        assert np.array_equal(hdr, want_h)
        assert all(vals[i, :hdr[i, 3]].tobytes() == want_v[i, :hdr[i, 3]].tobytes() for i in range(len(ref)))
    finally:
        hd.close()


def test_nms_in_argmax_mode():
    """pbd_set_nms suppresses the arg-max boxes: the kept list is Candidate.nonMaximaSuppression of the yardstick's records"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        im = synth.synthetic_frame(5, 72, 96)
        ref = records(hd, [im])
        fm = E.FrameMaps(flat, im, walk="argmax")
        want = ref.copy()
        for r in want:
            r[8:8 + 4 * r[6]] = yardstick_parts(flat, fm, r, np.float32).ravel()
        hd.set_walk(_lib.WALK_ARGMAX)
        for ov in (0.1, 0.5):
            hd.set_nms(ov)
            got = records(hd, [im])
            kept = mirror(want, 72, 96, ov)
            assert 0 < len(kept) < len(want)
            assert got.shape == kept.shape and np.array_equal(got, kept), ov
            assert not np.array_equal(kept, mirror(ref, 72, 96, ov))
    finally:
        hd.close()


def oracle_boxes(flat, im):
    """the part boxes (inclusive) of the oracle's best detection of im"""
    from oracle import oracle
    best = max(oracle.detect(flat, im), key=lambda r: r["score"])
    return [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best["parts"]]


def rect_passes(parts, boxes, overlap):
    return [bool(E.overlap_passes(tuple(np.asarray(v) for v in (x, y, x + w, y + h)), boxes[p], overlap))
            for p, (x, y, w, h) in enumerate(parts)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_latent_in_argmax_mode(dtype):
    """records and examples of pbd_detect_latent == latent_search(walk="argmax"); every part rectangle of every found record
    passes testoverlap, which the reference's composed walk does not give (frames and overlap chosen on the yardstick)"""
    model = M.synthetic_tiny_model(thresh=-100.0)
    flat = model.flatten()
    frames = [synth.synthetic_frame(12, 52, 44), synth.synthetic_frame(13, 36, 60), synth.synthetic_frame(22, 40, 40)]
    boxes = [oracle_boxes(flat, im) for im in frames]
    overlap = 0.7
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 16)
    try:
        ref, found = hd.detect_latent(frames, boxes, overlap)
        assert found.all()
        fails = sum(not all(rect_passes(r[8:8 + 4 * r[6]].reshape(-1, 4), boxes[f], overlap)) for f, r in enumerate(ref))
        assert fails >= 1
        hd.set_walk(_lib.WALK_ARGMAX)
        rec, found = hd.detect_latent(frames, boxes, overlap)
        hdr, vals = hd.examples(rec)
        from oracle import oracle
        for f, im in enumerate(frames):
            want = E.latent_search(model, im, boxes[f], overlap, None, dtype, walk="argmax")
            r = rec[f]
            assert (r[0], r[1], r[2], r[3], r[4]) == (f, want["component"], want["level"], want["root_x"], want["root_y"]), f
            assert r[5:6].view(np.float32)[0].tobytes() == np.float32(want["score"]).tobytes()
            assert r[6] == len(want["parts"]) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want["parts"])
            assert bool(found[f]) and want["found"]
            assert all(rect_passes(want["parts"], boxes[f], overlap)), f
            feats, _ = oracle.features_pyramid(flat, im, dtype)
            wh, wv = E.example(flat, feats[want["level"]], want["component"], want["placement"], f, dtype)
            assert np.array_equal(hdr[f], wh) and vals[f, :wh[3]].tobytes() == wv[:wh[3]].tobytes(), f
        # the twin followed its handle back as well
        hd.set_walk(_lib.WALK_REFERENCE)
        again, _ = hd.detect_latent(frames, boxes, overlap)
        assert np.array_equal(again, ref)
    finally:
        hd.close()


def test_python_mirror_and_refusals():
    model = M.synthetic_tiny_model(thresh=-1.0)
    im = synth.synthetic_frame(5, 72, 96)
    det = detector.PartsBasedDetector(device=0)
    det.setWalk("argmax")
    det.distributeModel(model)            # kept across distributeModel
    cands = det.detect(im)
    hdr, vals = det.examples(cands)
    w = det.modelVector()
    got = E.dot(hdr, vals, w)
    score = np.array([c.score() for c in cands])
    assert np.all(np.abs(got - score) <= E.rounding_bound(model.flatten(), hdr, vals, w) + np.abs(score) * 2.0 ** -24)
    det.setWalk("reference")
    hdr2, vals2 = det.examples(cands)
    assert np.any(E.dot(hdr2, vals2, w) < score - E.rounding_bound(model.flatten(), hdr2, vals2, w) - np.abs(score) * 2.0 ** -24)
    with pytest.raises(PbdError) as e:
        det.setWalk("best")
    assert e.value.code == -1
    hd = det.hd
    for mode in (-1, 2):
        with pytest.raises(PbdError) as e:
            hd.set_walk(mode)
        assert e.value.code == -1
    f = np.ascontiguousarray(im)
    arr = _lib.ptr_array([f])
    hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 1, arr, f.shape[0], f.shape[1], f.shape[2], f.shape[1] * f.shape[2]))
    try:
        with pytest.raises(PbdError) as e:
            hd.set_walk(_lib.WALK_ARGMAX)
        assert e.value.code == -5
    finally:
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        n = C.c_int()
        hd.check(hd.lib.pbd_detect_batch_wait(hd.h, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    hd.set_walk(_lib.WALK_ARGMAX)
    hd.close()
