"""Training examples on the device (pbd_model_vector, pbd_examples*), bit for bit against the numpy yardstick in
partsbaseddetector_amd/examples.py (walked through the oracle's own maps) in PBD_CONV_EXACT, for float and double: the person
model, a multi-component model, shared filter ids, windows that cross the map border, records after pbd_set_nms, a mixed-size
pbd_detect_frames batch; the device form against the host form; the score identity; refusals."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def shared_model():
    """tiny model whose part 2 uses part 1's filters (a filter id twice inside a component: the sequential schedule)"""
    m = M.synthetic_tiny_model(thresh=-1.0)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def records(hd, frames, depth=False):
    """the records of one pbd_detect_frames call (n, stride)"""
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], _lib.DEPTH_CODE[fr[0].dtype], buf.ctypes.data,
                                      hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def check_against_yardstick(hd, flat, frames, rec, dtype, w=None, some_exact=True):
    """host examples of rec == the yardstick's, bit for bit; the score identity on every example: w . x is the placement's own
    score within the rounding bound, and at most the record's score (equal to it, within the bound, where the composed
    pointers are the transform's arg-max: some of a small model's records; with 26 parts almost never)"""
    hdr, vals = hd.examples(rec)
    maps = [E.FrameMaps(flat, f, dtype) for f in frames]
    want_h, want_v = E.examples_of_records(flat, maps, rec, 0, dtype)
    assert np.array_equal(hdr, want_h)
    for i in range(len(rec)):
        n = int(hdr[i, 3])
        assert vals[i, :n].tobytes() == want_v[i, :n].tobytes(), i
    w = hd.model_vector() if w is None else w
    assert w.tobytes() == E.model_vector(flat, dtype).tobytes()
    got = E.dot(hdr, vals, w)
    bound = E.rounding_bound(flat, hdr, vals, w, dtype)
    score = rec[:, 5].view(np.float32).astype(np.float64)
    exact = 0
    for i, r in enumerate(rec):
        fm = maps[int(r[0])]
        pl = fm.placement(int(r[2]), int(r[1]), int(r[3]), int(r[4]))
        ps = E.placement_score(flat, fm.resp(int(r[2])), int(r[1]), pl)
        assert abs(got[i] - ps) <= bound[i], (i, got[i], ps, bound[i])
        # the record's score is rounded to float (Candidate::confidence_): half an ulp of it on top
        slack = bound[i] + abs(score[i]) * 2.0 ** -24
        assert got[i] <= score[i] + slack
        exact += abs(got[i] - score[i]) <= slack
    assert exact > 0 or not some_exact
    return hdr, vals


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_and_shared_filters_bit_for_bit(dtype):
    for model in (M.synthetic_tiny_model(thresh=-1.0), shared_model()):
        flat = model.flatten()
        hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
        try:
            im = synth.synthetic_frame(5, 72, 96)
            rec = records(hd, [im])
            assert len(rec) > 20
            hdr, _ = check_against_yardstick(hd, flat, [im], rec, dtype)
            # windows crossing the map border (the 0 / 1 padding) were among them
            assert any((r[3] < 2 or r[4] < 2) for r in rec)
        finally:
            hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_person_model_subset_any_order(dtype):
    model = M.synthetic_person_model(thresh=-100.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18)
    try:
        im = synth.synthetic_frame(2, 120, 160)
        rec = records(hd, [im])
        assert len(rec) > 100
        rng = np.random.default_rng(1)
        sub = rec[rng.permutation(len(rec))[:150]]
        check_against_yardstick(hd, flat, [im], sub, dtype, some_exact=False)
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wide_map_int16_planes_bit_for_bit(dtype):
    """A map wider than 256 cells: the position planes are int16, so the walk of pbd_examples is k_ex_walk<R, int16_t>, which
    no other frame of this file or of test_gpu_latent.py reaches.  36 x 1100 pixels: the tiny model's pyramid plan refuses a
    frame of 24 or 32 rows at that width (level 0 is 7 x 273 cells); seed and threshold were chosen with the oracle so that a few
    hundred records pass and some of them walk to a part beyond column 255, where a wrong index into the transposed IxRaw
    plane cannot give the right position."""
    model = M.synthetic_tiny_model(thresh=0.8)
    flat = model.flatten()
    im = synth.synthetic_frame(13, 36, 1100)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 12)
    try:
        assert int(hd.plan(36, 1100)["feat_cols"].max()) > 256
        rec = records(hd, [im])
        assert 100 <= len(rec) <= 600
        check_against_yardstick(hd, flat, [im], rec, dtype, some_exact=False)
        fm = E.FrameMaps(flat, im, dtype)
        walked = [fm.placement(int(r[2]), int(r[1]), int(r[3]), int(r[4])) for r in rec]
        assert any(x >= 256 for pl in walked for (x, _, _) in pl[1:])
    finally:
        hd.close()


def test_multi_component_mixed_batch_and_nms():
    model = M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0)
    flat = model.flatten()
    hd = detector.Handle(model, device=0, max_batch=4, max_candidates=1 << 18)
    try:
        frames = [synth.synthetic_frame(3, 64, 80), synth.synthetic_frame(4, 96, 72), synth.synthetic_frame(6, 50, 130)]
        rec = records(hd, frames)
        assert len(set(rec[:, 0])) == 3 and len(set(rec[:, 1])) == 3
        sub = rec[np.random.default_rng(2).permutation(len(rec))[:300]]
        check_against_yardstick(hd, flat, frames, sub, np.float32, some_exact=False)
        hd.set_nms(0.3)
        kept = records(hd, frames)
        assert 0 < len(kept) < len(rec)
        check_against_yardstick(hd, flat, frames, kept, np.float32, some_exact=False)
    finally:
        hd.close()


def test_device_form_equals_host_form():
    import torch
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        im = synth.synthetic_frame(7, 80, 100)
        rec = records(hd, [im])
        hw, vw = hd.example_stride()
        hdr, vals = hd.examples(rec)
        bad = rec[:3].copy()
        bad[1, 3] = 10000                        # root outside the map
        allrec = np.concatenate([rec, bad])
        cap = len(allrec) + 5
        pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
        pay[0] = len(allrec)
        pay[1:1 + allrec.size] = torch.from_numpy(allrec.ravel()).cuda()
        d_hdr = torch.full((cap, hw), -7, dtype=torch.int32, device="cuda")
        d_val = torch.zeros((cap, vw), dtype=torch.float32, device="cuda")
        hd.examples_device(pay.data_ptr(), cap, 0, d_hdr.data_ptr(), d_val.data_ptr())
        hd.check(hd.lib.pbd_synchronize(hd.h))
        gh, gv = d_hdr.cpu().numpy(), d_val.cpu().numpy()
        n = len(rec)
        assert np.array_equal(gh[:n], hdr)
        for i in range(n):
            k = int(hdr[i, 3])
            assert gv[i, :k].tobytes() == vals[i, :k].tobytes()
        assert np.array_equal(gh[n:n + 3, 2], [hdr[0, 2], -1, hdr[2, 2]])
        assert gh[n + 1, 0] == n + 1 and np.all(gh[n + 1, 3:] == 0)
        assert np.all(gh[n + 3:] == -7)           # past the count: untouched
        # a -1 payload (a suppression overflow) writes nothing
        pay[0] = -1
        d_hdr.fill_(-7)
        hd.examples_device(pay.data_ptr(), cap, 0, d_hdr.data_ptr(), d_val.data_ptr())
        hd.check(hd.lib.pbd_synchronize(hd.h))
        assert bool((d_hdr == -7).all())
        # the resident result is left as it was: a detect afterwards equals one before
        again = records(hd, [im])
        assert np.array_equal(again, rec)
    finally:
        hd.close()


def test_refusals():
    model = M.synthetic_tiny_model(thresh=-1.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        rec0 = np.zeros((1, hd.stride), np.int32)
        with pytest.raises(PbdError) as e:
            hd.examples(rec0)
        assert e.value.code == -5                 # no resident result
        im = synth.synthetic_frame(5, 72, 96)
        rec = records(hd, [im])
        for field, value in ((0, 1), (2, 99), (1, 5), (3, -1), (4, 10000)):
            bad = rec[:4].copy()
            bad[2, field] = value
            with pytest.raises(PbdError) as e:
                hd.examples(bad)
            assert e.value.code == -1 and "record 2" in str(e.value)
        hdr, _ = hd.examples(rec[:0])
        assert hdr.shape[0] == 0
        # after setFilters() the responses and the DP result are gone
        flat = model.flatten()
        filt = [np.ascontiguousarray(f, np.float32) for f in model.filtersw]
        arr = _lib.ptr_array(filt)
        ks = np.array(flat.filter_ksize, np.int32)
        hd.check(hd.lib.pbd_conv_set_filters(hd.h, len(filt), arr, _lib.ptr(ks, C.c_int)))
        with pytest.raises(PbdError) as e:
            hd.examples(rec[:1])
        assert e.value.code == -5
    finally:
        hd.close()


def test_python_mirror():
    model = M.synthetic_tiny_model(thresh=-1.0)
    det = detector.PartsBasedDetector(device=0)
    det.distributeModel(model)
    im = synth.synthetic_frame(5, 72, 96)
    cands = det.detect(im)
    w = det.modelVector()
    assert w.tobytes() == model.to_vector().tobytes()
    hdr, vals = det.examples(cands)
    got = E.dot(hdr, vals, w)
    assert len(got) == len(cands)
    assert np.all(got <= np.array([c.score() for c in cands]) + E.rounding_bound(model.flatten(), hdr, vals, w) + 1e-5)
    dense = E.densify(hdr, vals, len(w))
    np.testing.assert_allclose(dense @ w.astype(np.float64), got, rtol=0, atol=1e-9)
    # distributeModel accepts the model from its own vector, and detects the same
    det2 = detector.PartsBasedDetector(device=0)
    det2.distributeModel(model.from_vector(w))
    again = det2.detect(im)
    assert [(c.level, c.component, c.root, c.score()) for c in again] == [(c.level, c.component, c.root, c.score()) for c in cands]
