"""Latent positives on the device (pbd_detect_latent) bit for bit against the numpy yardstick (examples.latent_search, on the
oracle) in PBD_CONV_EXACT for float and double: mixed frame sizes, fixed mixtures, shared filter ids, several components, boxes off
the image; a normal detect afterwards; the examples of the positives; refusals."""
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
    m = M.synthetic_tiny_model(thresh=-100.0)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def boxes_of(hd, im):
    """the part boxes (inclusive) of the handle's best detection of im"""
    rec = hd.unpack_candidates(*_detect(hd, im))
    best = max(rec, key=lambda c: c.score())
    return [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts]


def _detect(hd, im):
    import ctypes as C
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    im = np.ascontiguousarray(im)
    hd.check(hd.lib.pbd_detect(hd.h, im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], im.strides[0], buf.ctypes.data,
                               hd.max_candidates, C.byref(n)))
    return buf, n.value


def check(hd, model, frames, boxes, overlap, mixtures, dtype):
    rec, found = hd.detect_latent(frames, boxes, overlap, mixtures)
    for f, im in enumerate(frames):
        want = E.latent_search(model, im, boxes[f], overlap, None if mixtures is None else mixtures[f], dtype)
        r = rec[f]
        assert (r[0], r[1], r[2], r[3], r[4]) == (f, want["component"], want["level"], want["root_x"], want["root_y"]), f
        assert r[5:6].view(np.float32)[0].tobytes() == np.float32(want["score"]).tobytes()
        assert r[6] == len(want["parts"]) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want["parts"])
        assert bool(found[f]) == want["found"]
    return rec, found


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_mixed_frames_and_fixed_mixtures(dtype):
    model = M.synthetic_tiny_model(thresh=-100.0)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 16)
    try:
        frames = [synth.synthetic_frame(11, 40, 56), synth.synthetic_frame(12, 52, 44), synth.synthetic_frame(13, 36, 60)]
        boxes = [boxes_of(hd, im) for im in frames]
        boxes[2] = [(5000, 5000, 5040, 5040)] * 3            # off the image: nothing passes
        rec, found = check(hd, model, frames, boxes, 0.3, None, dtype)
        assert list(found) == [1, 1, 0]
        check(hd, model, frames, boxes, 0.5, [[1, -1, 0], [0, 1, -1], [-1, -1, -1]], dtype)
        # the positives' feature vectors (offsets in this handle's model vector): w . x at most the score
        hdr, vals = hd.examples(rec[:2])
        w = hd.model_vector()
        got = E.dot(hdr, vals, w)
        assert np.all(got <= rec[:2, 5].view(np.float32) + E.rounding_bound(model.flatten(), hdr, vals, w, dtype) + 1e-4)
        # a normal detect afterwards equals a fresh handle's
        fresh = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
        try:
            a, na = _detect(hd, frames[0])
            b, nb = _detect(fresh, frames[0])
            assert na == nb and np.array_equal(a[:na * hd.stride], b[:nb * hd.stride])
        finally:
            fresh.close()
    finally:
        hd.close()


def test_shared_filters_and_components():
    for model in (shared_model(), M.synthetic_face_model(nparts=5, ncomponents=3, thresh=-100.0)):
        hd = detector.Handle(model, device=0, max_batch=2, max_candidates=1 << 16)
        try:
            frames = [synth.synthetic_frame(21, 48, 64), synth.synthetic_frame(22, 40, 40)]
            boxes = [boxes_of(hd, im) for im in frames]
            rec, found = check(hd, model, frames, boxes, 0.3, None, np.float32)
            assert found.all()
        finally:
            hd.close()


def test_refusals():
    m = M.synthetic_tiny_model(thresh=-100.0)
    m.filterid.append([list(x) for x in m.filterid[0][:2]])
    m.biasid.append([list(x) for x in m.biasid[0][:2]])
    m.defid.append([list(x) for x in m.defid[0][:2]])
    m.parentid.append(list(m.parentid[0][:2]))
    im = synth.synthetic_frame(3, 40, 56)
    hd = detector.Handle(m, device=0)
    try:
        with pytest.raises(PbdError) as e:
            hd.detect_latent([im], [[(0, 0, 9, 9)] * 3], 0.5)
        assert e.value.code == -2
    finally:
        hd.close()
    hd = detector.Handle(M.synthetic_tiny_model(), device=0)
    try:
        with pytest.raises(PbdError) as e:
            hd.detect_latent([im], [[(0, 0, 9, 9)] * 3], float("nan"))
        assert e.value.code == -1
        hd.set_level_shard(0, 2)
        with pytest.raises(PbdError) as e:
            hd.detect_latent([im], [[(0, 0, 9, 9)] * 3], 0.5)
        assert e.value.code == -2
    finally:
        hd.close()


def test_examples_on_a_level_sharded_handle():
    """a sharded rank works on its own levels; a record of another rank's level is PBD_ERR_INVALID"""
    model = M.synthetic_tiny_model(thresh=-100.0)
    hd = detector.Handle(model, device=0, max_candidates=1 << 16)
    try:
        hd.set_level_shard(0, 2)
        im = synth.synthetic_frame(5, 72, 96)
        buf, n = _detect(hd, im)
        rec = buf[:n * hd.stride].reshape(n, hd.stride)
        assert n > 0
        hdr, vals = hd.examples(rec)
        want_h, want_v = E.examples_of_records(model.flatten(), [E.FrameMaps(model.flatten(), im)], rec)
        assert np.array_equal(hdr, want_h)
        plan = hd.plan(72, 96)
        foreign = [l for l in range(plan["nlevels"]) if plan["feat_rows"][l] == 0]
        assert foreign
        bad = rec[:1].copy()
        bad[0, 2], bad[0, 3], bad[0, 4] = foreign[0], 0, 0
        with pytest.raises(PbdError) as e:
            hd.examples(bad)
        assert e.value.code == -1
    finally:
        hd.close()
