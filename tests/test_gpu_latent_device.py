"""pbd_detect_latent_device -- latent positives of frames already on the device -- against pbd_detect_latent on the same frames:
the records, found, the examples of the positives and the root planes of every level, byte for byte, for float and double, a
mixed-size batch, fixed mixtures and frames given as regions of one larger device image; the refusals of the host form.
pbd_detect_latent itself is pinned on the yardstick by tests/test_gpu_latent.py."""
import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
SIZES = ((40, 56), (52, 44), (36, 60))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def frames_u8():
    return [synth.synthetic_frame(11 + i, r, c) for i, (r, c) in enumerate(SIZES)]


def boxes_of(hd, frames):
    """per frame the part boxes (inclusive) of the handle's best detection"""
    import ctypes as C
    out = []
    for im in frames:
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        n = C.c_int()
        im = np.ascontiguousarray(im)
        hd.check(hd.lib.pbd_detect(hd.h, im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], im.strides[0], buf.ctypes.data,
                                   hd.max_candidates, C.byref(n)))
        best = max(hd.unpack_candidates(buf, n.value), key=lambda c: c.score())
        out.append([(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts])
    return out


def snapshot(hd, rec, found, sizes):
    """everything a latent call leaves: records, found, the examples of every record, the root planes of every level"""
    hdr, vals = hd.examples(rec)
    planes = []
    for f, (r, c) in enumerate(sizes):
        plan = hd.plan(r, c)
        for l in range(plan["nlevels"]):
            fr, fc = int(plan["feat_rows"][l]), int(plan["feat_cols"][l])
            if fr > 0 and fc > 0:
                planes.append(hd.get_stage(_lib.STAGE_ROOTV, f, l, fr, fc).tobytes())
                planes.append(hd.get_stage(_lib.STAGE_ROOTI, f, l, fr, fc).tobytes())
    return rec.tobytes(), found.tobytes(), hdr.tobytes(), vals.tobytes(), planes


def region_views(frames):
    """the frames as views of ONE device image (foreign pixels between them), and contiguous uploads of the same frames"""
    import torch
    big = np.full((120, 200, frames[0].shape[2]), 99, frames[0].dtype)
    at = ((3, 5), (50, 9), (60, 120))
    for (y, x), f in zip(at, frames):
        big[y:y + f.shape[0], x:x + f.shape[1]] = f
    d_big = torch.from_numpy(big).cuda()
    views = [d_big[y:y + f.shape[0], x:x + f.shape[1]] for (y, x), f in zip(at, frames)]
    assert not any(v.is_contiguous() for v in views)
    return views, [torch.from_numpy(np.array(f)).cuda() for f in frames]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_form_equals_host_form(dtype):
    import torch
    model = M.synthetic_tiny_model(thresh=-100.0)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_batch=4, max_candidates=1 << 16)
    try:
        frames = frames_u8()
        boxes = boxes_of(hd, frames)
        boxes[2] = [(5000, 5000, 5040, 5040)] * 3            # off the image: nothing passes
        views, dense = region_views(frames)
        torch.cuda.synchronize()
        for overlap, mix in ((0.3, None), (0.5, [[1, -1, 0], [0, 1, -1], [-1, -1, -1]])):
            rec, found = hd.detect_latent(frames, boxes, overlap, mix)
            want = snapshot(hd, rec, found, SIZES)
            if mix is None:
                assert list(found) == [1, 1, 0]
            for d_frames in (views, dense):
                descs, cn, code = detector.device_frames(d_frames)
                assert (cn, code) == (3, 0)
                rec2, found2 = hd.detect_latent_device(descs, cn, code, boxes, overlap, mix)
                got = snapshot(hd, rec2, found2, SIZES)
                assert got[:4] == want[:4]
                assert len(got[4]) == len(want[4]) > 6 and got[4] == want[4]
    finally:
        hd.close()


@pytest.mark.parametrize("pix", [np.uint16, np.float32, np.float64])
def test_other_depths_and_one_channel(pix):
    import torch
    model = M.synthetic_tiny_model(thresh=-100.0)
    hd = detector.Handle(model, device=0, max_batch=2, max_candidates=1 << 16)
    try:
        u8 = frames_u8()[:2]
        boxes = boxes_of(hd, u8)
        frames = [np.ascontiguousarray((f[:, :, :1].astype(np.float64) * (257 if pix == np.uint16 else 1 / 255)).astype(pix)) for f in u8]
        rec, found = hd.detect_latent(frames, boxes, 0.0)
        want = snapshot(hd, rec, found, SIZES[:2])
        views, _ = region_views(frames)
        torch.cuda.synchronize()
        descs, cn, code = detector.device_frames(views)
        assert (cn, code) == (1, _lib.DEPTH_CODE[np.dtype(pix)])
        rec2, found2 = hd.detect_latent_device(descs, cn, code, boxes, 0.0)
        assert snapshot(hd, rec2, found2, SIZES[:2]) == want
    finally:
        hd.close()


def test_detector_takes_device_tensors():
    """PartsBasedDetector.detectLatent on torch tensors (views included) gives the candidates of the same host arrays"""
    model = M.synthetic_tiny_model(thresh=-100.0)
    det = detector.PartsBasedDetector(max_batch=4, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        frames = frames_u8()
        boxes = boxes_of(det.hd, frames)
        want, wfound = det.detectLatent(frames, boxes, 0.3)
        views, dense = region_views(frames)
        for d_frames in (views, dense):
            got, found = det.detectLatent(d_frames, boxes, 0.3)
            assert list(found) == list(wfound) and wfound.all()
            for g, w in zip(got, want):
                assert (g.frame, g.level, g.component, tuple(g.root)) == (w.frame, w.level, w.component, tuple(w.root))
                assert np.array_equal(g.parts, w.parts) and np.float32(g.score()).tobytes() == np.float32(w.score()).tobytes()
        one, f1 = det.detectLatent(views[1], boxes[1:2], 0.3)                 # a single tensor is one frame
        assert len(one) == 1 and f1[0] and np.array_equal(one[0].parts, want[1].parts)
    finally:
        det.hd.close()


def test_refusals():
    import torch
    im = synth.synthetic_frame(3, 40, 56)
    d_im = torch.from_numpy(im).cuda()
    torch.cuda.synchronize()
    desc = [(d_im.data_ptr(), 40, 56, 56 * 3)]
    box = [[(0, 0, 9, 9)] * 3]
    m = M.synthetic_tiny_model(thresh=-100.0)
    m.filterid.append([list(x) for x in m.filterid[0][:2]])
    m.biasid.append([list(x) for x in m.biasid[0][:2]])
    m.defid.append([list(x) for x in m.defid[0][:2]])
    m.parentid.append(list(m.parentid[0][:2]))
    hd = detector.Handle(m, device=0)
    try:
        with pytest.raises(PbdError) as e:
            hd.detect_latent_device(desc, 3, 0, box, 0.5)            # components with different part counts
        assert e.value.code == -2
    finally:
        hd.close()
    det = detector.PartsBasedDetector(max_batch=2)
    det.distributeModel(M.synthetic_tiny_model(thresh=-100.0))
    hd = det.hd
    try:
        rec, found = hd.detect_latent([im], box, 0.5)
        before = hd.examples(rec)
        for args, code in (((desc, 3, 0, box, float("nan")), -1),                                  # NaN overlap
                           (([(0, 40, 56, 168)], 3, 0, box, 0.5), -1),                             # a null frame
                           (([(d_im.data_ptr(), 40, 56, 167)], 3, 0, box, 0.5), -1),               # a pitch below the row
                           (([(d_im.data_ptr(), 0, 56, 168)], 3, 0, box, 0.5), -1),                # an empty frame
                           ((desc, 2, 0, box, 0.5), -1),                                           # channels
                           ((desc, 3, 3, box, 0.5), -2),                                           # depth code
                           (([(d_im.data_ptr() + 1, 20, 27, 168)], 1, 2, box, 0.5), -1),           # a misaligned 16-bit frame
                           ((desc * 3, 3, 0, box * 3, 0.5), -1)):                                  # more frames than max_batch
            with pytest.raises(PbdError) as e:
                hd.detect_latent_device(*args)
            assert e.value.code == code, args
        bx, cand, fnd = np.zeros(12, np.int32), np.zeros(hd.stride, np.int32), np.zeros(1, np.int32)
        for null in (2, 5, 8, 9):                                                                   # frames, boxes, cand, found
            a = [hd.h, 1, _lib.frame_array(desc), 3, 0, bx.ctypes.data, None, 0.5, cand.ctypes.data, fnd.ctypes.data]
            a[null] = None
            assert hd.lib.pbd_detect_latent_device(*a) == -1
        after = hd.examples(rec)                                                                    # the resident result stayed
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        det.submit_batch([im])
        with pytest.raises(PbdError) as e:
            hd.detect_latent_device(desc, 3, 0, box, 0.5)
        assert e.value.code == -5
        det.wait_batch()
        hd.detect_latent_device(desc, 3, 0, box, 0.5)
        hd.set_level_shard(0, 2)
        with pytest.raises(PbdError) as e:
            hd.detect_latent_device(desc, 3, 0, box, 0.5)
        assert e.value.code == -2
    finally:
        hd.close()
