"""Augmented positives on the device (pbd_augment_frames*): every comparison is byte equality (tobytes())
against the numpy yardstick partsbaseddetector_amd/augment.py, fed the coefficients pbd_augment_plan reports.

Frames and angles are those of tests/augment_cases.py: 1 x 1, 2 x 3, 5 x 4, 17 x 9, 48 x 64 and 70 x 130 (destination rows of more
than two waves), degrees 0, 90, 180, 270, +-7.5, +-15, 45, 33.3, mirror off
and on, channels 1 and 3, the four depths.  Every destination of the device calls has a padded pitch and is pre-filled with a
sentinel byte: the padding must keep it and the zero fill must replace it."""
import ctypes as C
import functools

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import augment as A
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

import augment_cases as AC

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 48             # bytes behind every destination row: a multiple of every element size


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def hd():
    h = detector.Handle(M.synthetic_tiny_model(thresh=-1e9), device=0, max_batch=4)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def reference(dtype, cn, jobs):
    """the yardstick's copies of `jobs` over AC.frames(dtype, cn), with the library's coefficients"""
    fr = AC.frames(dtype, cn)
    out = []
    for f, m, d in jobs:
        coef = A.plan_c(fr[f].shape[0], fr[f].shape[1], d)[2]
        out.append(A.rotate_ref(fr[f], d, m, coef if d else None))
    return tuple(out)


def upload(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]      # np.array: a writable, contiguous copy


def padded_destinations(shapes, itemsize, cn):
    """one sentinel-filled byte tensor (rows, row bytes + PAD) per destination, and its descriptor"""
    import torch
    bufs = [torch.full((r, c * cn * itemsize + PAD), SENTINEL, dtype=torch.uint8, device="cuda") for r, c in shapes]
    return bufs, [(b.data_ptr(), r, c, b.shape[1]) for b, (r, c) in zip(bufs, shapes)]


def check_destinations(bufs, want):
    import torch
    torch.cuda.synchronize()
    for i, (b, w) in enumerate(zip(bufs, want)):
        got = b.cpu().numpy()
        rb = w.shape[1] * w.shape[2] * w.itemsize
        assert got[:, :rb].tobytes() == w.tobytes(), i
        assert (got[:, rb:] == SENTINEL).all(), i


def device_call(hd, d_frames, cn, dtype, jobs, want):
    descs = [(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * t.element_size()) for t in d_frames]
    bufs, odesc = padded_destinations([w.shape[:2] for w in want], np.dtype(dtype).itemsize, cn)
    hd.augment_frames_device(descs, cn, _lib.DEPTH_CODE[np.dtype(dtype)], jobs, odesc)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    check_destinations(bufs, want)


# ---- every shape, angle, depth and channel count in one call ----------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_one_call_many_jobs(hd, dtype, cn):
    """120 jobs over six frames in one launch; the yardstick's zero fill is present (so the sentinel had to be overwritten)"""
    jobs = tuple(AC.all_jobs())
    want = reference(dtype, cn, jobs)
    assert any((w.reshape(-1, cn) == 0).all(axis=1).any() for w in want)
    assert want[-1].shape[1] > 128 and max(w.shape[0] for w in want) > 128      # rows of > 2 waves, > 16 row tiles
    device_call(hd, upload(AC.frames(dtype, cn)), cn, dtype, jobs, want)


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 1), (np.float64, 3)])
def test_rows_longer_than_one_tile(hd, dtype, cn):
    """3 x 300: destination rows of 300 and 301 pixels take two 256-pixel tiles, the quarter turn's 301 rows 38 row tiles"""
    im = (np.random.default_rng(8).integers(1, 256, (3, 300, cn))).astype(dtype)
    jobs = ((0, False, 0.0), (0, True, 0.0), (0, False, 7.5), (0, True, 90.0), (0, False, 180.0))
    want = [A.rotate_ref(im, d, m, A.plan_c(3, 300, d)[2] if d else None) for _, m, d in jobs]
    assert want[2].shape[1] > 256 and want[3].shape[0] > 256
    device_call(hd, upload([im]), cn, dtype, jobs, want)


def test_a_frame_without_a_job_and_three_jobs_on_one_frame(hd):
    jobs = ((3, False, 15.0), (3, True, 15.0), (0, False, 45.0), (3, True, 0.0), (5, False, -7.5))      # frames 1, 2 and 4: none
    device_call(hd, upload(AC.frames(np.uint8, 3)), 3, np.uint8, jobs, reference(np.uint8, 3, jobs))


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_source_is_a_region_of_a_larger_device_image(hd, dtype):
    """the 48 x 64 and 17 x 9 frames stand inside one 80 x 100 device image whose other pixels would show in a wrong read"""
    import torch
    fr = AC.frames(dtype, 3)
    big = np.full((80, 100, 3), 77, dtype)
    big[5:53, 7:71] = fr[4]
    big[60:77, 90:99] = fr[3]
    d_big = torch.from_numpy(big).cuda()
    views = {4: d_big[5:53, 7:71], 3: d_big[60:77, 90:99]}
    d_frames = [views.get(i, t) for i, t in enumerate(upload(fr))]
    assert d_frames[4].stride(0) == 300 and not d_frames[4].is_contiguous()
    jobs = tuple((f, m, d) for f in (3, 4) for d in (0.0, 90.0, 33.3, -15.0) for m in (False, True))
    device_call(hd, d_frames, 3, dtype, jobs, reference(dtype, 3, jobs))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_host_form_equals_device_form(hd, dtype, cn):
    """host frames with padded rows in, host destinations with padded rows out; the padding keeps its sentinel"""
    fr = AC.frames(dtype, cn)
    jobs = tuple((f, m, d) for f in range(len(fr)) for d in (0.0, 90.0, 45.0, -7.5) for m in (False, True))
    want = reference(dtype, cn, jobs)
    padded = []
    for f in fr:                                                      # every source row followed by 5 foreign pixels
        p = np.full((f.shape[0], f.shape[1] + 5, cn), 9, f.dtype)
        p[:, :f.shape[1]] = f
        padded.append(p[:, :f.shape[1]])
    outs, views = [], []
    for w in want:
        o = np.full((w.shape[0], w.shape[1] * cn * w.itemsize + PAD), SENTINEL, np.uint8)
        outs.append(o)
        views.append(o[:, :w.shape[1] * cn * w.itemsize].view(w.dtype).reshape(w.shape[0], w.shape[1], cn))
    descs = _lib.frame_array([(p.ctypes.data, p.shape[0], p.shape[1], p.strides[0]) for p in padded])
    odesc = _lib.frame_array([(v.ctypes.data, v.shape[0], v.shape[1], v.strides[0]) for v in views])
    hd.check(hd.lib.pbd_augment_frames(hd.h, len(padded), descs, cn, _lib.DEPTH_CODE[np.dtype(dtype)], len(jobs),
                                       _lib.augment_array(jobs), odesc))
    for i, (o, v, w) in enumerate(zip(outs, views, want)):
        assert v.tobytes() == w.tobytes(), i
        assert (o[:, w.shape[1] * cn * w.itemsize:] == SENTINEL).all(), i
    got = hd.augment_frames(list(fr), jobs)                           # the binding's own destinations
    assert all(g.tobytes() == w.tobytes() and g.shape == w.shape for g, w in zip(got, want))


def test_detector_augment_frames_and_augment_positives():
    """PartsBasedDetector.augmentFrames on host arrays and on device tensors; augment_positives against augment_positives_ref"""
    import torch
    det = detector.PartsBasedDetector()
    det.distributeModel(M.synthetic_tiny_model())
    try:
        fr = AC.frames(np.uint8, 3)
        jobs = tuple((f, m, d) for f in (1, 3, 5) for d in (0.0, 15.0) for m in (False, True))
        want = reference(np.uint8, 3, jobs)
        for frames in (list(fr), upload(fr)):
            got = det.augmentFrames(frames, jobs)
            assert all(g.is_cuda and g.cpu().numpy().tobytes() == w.tobytes() and tuple(g.shape) == w.shape for g, w in zip(got, want))
        gray = det.augmentFrames([fr[3][:, :, 0]], [(0, True, 15.0)])[0]
        assert gray.ndim == 2 and gray.cpu().numpy().tobytes() == A.rotate_ref(fr[3][:, :, 0], 15.0, True, A.plan_c(17, 9, 15.0)[2]).tobytes()
        assert det.augmentFrames(list(fr), []) == []
    finally:
        det.hd.close()
    pos = [{"im": fr[3], "points": np.array([[1.0, 2.0], [3.5, 4.0], [7.0, 16.0]])},
           {"im": np.ascontiguousarray(AC.frames(np.float32, 1)[4][:, :, 0]), "points": np.array([[0.0, 0.0], [63.0, 47.0], [10.0, 5.5]])}]
    got = A.augment_positives(pos, (15.0, -33.3), [0, 2, 1], device=0)
    want = A.augment_positives_ref(pos, (15.0, -33.3), [0, 2, 1], coef_of=lambda d: A.plan_c(4, 4, d)[2])
    assert len(got) == len(want) == 12
    for g, w in zip(got, want):
        assert g["im"].is_cuda and tuple(g["im"].shape) == w["im"].shape and g["im"].cpu().numpy().tobytes() == w["im"].tobytes()
        assert g["points"].tobytes() == w["points"].tobytes()


def test_points_equal_the_yardstick():
    rng = np.random.default_rng(6)
    for r, c in AC.SHAPES:
        pts = rng.uniform(-4, 140, (16, 2))
        for d in AC.DEGREES:
            coef = A.plan_c(r, c, d)[2]
            for m in (False, True):
                assert A.points_c(pts, r, c, d, m).tobytes() == A.points_ref(pts, r, c, d, m, coef if d else None).tobytes()


# ---- refusals, the resident result and the detect path ----------------------------------------------------------------------
def records(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], _lib.DEPTH_CODE[fr[0].dtype], buf.ctypes.data,
                                      hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def test_refusals_leave_destinations_and_resident_result(hd):
    import torch
    scene = [synth.synthetic_frame(71, 80, 96), synth.synthetic_frame(72, 64, 72)]
    before = records(hd, scene)
    assert len(before) >= 4
    ex_before = hd.examples(before[:4])
    fr = AC.frames(np.uint8, 3)
    d_fr = upload(fr)
    descs = [(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * t.element_size()) for t in d_fr]
    jobs = [(3, False, 15.0), (4, True, 90.0)]
    shapes = [A.plan_c(fr[f].shape[0], fr[f].shape[1], d)[:2] for f, _, d in jobs]
    bufs, odesc = padded_destinations(shapes, 1, 3)

    def call(descs=descs, cn=3, code=0, jobs=jobs, odesc=odesc, fn=None, njobs=None):
        fn = fn or hd.lib.pbd_augment_frames_device
        return fn(hd.h, len(descs), _lib.frame_array(descs), cn, code, len(jobs) if njobs is None else njobs, _lib.augment_array(jobs),
                  _lib.frame_array(odesc))

    bad = {
        "frame index above": (dict(jobs=[jobs[0], (6, False, 0.0)]), -1, "job 1"),
        "frame index below": (dict(jobs=[(-1, False, 0.0), jobs[1]]), -1, "job 0"),
        "nan degrees": (dict(jobs=[jobs[0], (4, True, float("nan"))]), -1, "job 1"),
        "inf degrees": (dict(jobs=[(3, False, float("inf")), jobs[1]]), -1, "job 0"),
        "destination rows": (dict(odesc=[(odesc[0][0], odesc[0][1] + 1, odesc[0][2], odesc[0][3]), odesc[1]]), -1, "job 0"),
        "destination cols": (dict(odesc=[odesc[0], (odesc[1][0], odesc[1][1], odesc[1][2] - 1, odesc[1][3])]), -1, "job 1"),
        "destination pitch": (dict(odesc=[odesc[0], (odesc[1][0], odesc[1][1], odesc[1][2], odesc[1][2] * 3 - 1)]), -1, "job 1"),
        "destination is a source": (dict(odesc=[odesc[0], (descs[4][0], odesc[1][1], odesc[1][2], odesc[1][3])]), -1, "job 1"),
        "null frame": (dict(descs=[descs[0], (0, 2, 3, 9)] + descs[2:]), -1, "frame 1"),
        "frame pitch": (dict(descs=descs[:5] + [(descs[5][0], 70, 130, 389)]), -1, "frame 5"),
        "channels": (dict(cn=2), -1, "channels"),
        "depth code": (dict(code=3), -2, "depth"),
        "negative njobs": (dict(njobs=-1), -1, "njobs"),
    }
    for name, (kw, code, word) in bad.items():
        assert call(**kw) == code, name
        assert word in hd.lib.pbd_last_error(hd.h).decode(), (name, hd.lib.pbd_last_error(hd.h))
    # a misaligned device destination (16-bit frames), and the host form's own refusals
    d16 = upload(AC.frames(np.uint16, 3))
    descs16 = [(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * 2) for t in d16]
    assert call(descs=descs16, code=2, odesc=[(odesc[0][0] + 1, odesc[0][1], odesc[0][2], odesc[0][3] + 400), odesc[1]]) == -1
    assert "job 0" in hd.lib.pbd_last_error(hd.h).decode()
    host_out = [np.full((r, c, 3), SENTINEL, np.uint8) for r, c in shapes]
    hdesc = [(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr]
    hodesc = [(o.ctypes.data, o.shape[0], o.shape[1], o.strides[0]) for o in host_out]
    assert call(descs=hdesc, odesc=[hodesc[0], (hdesc[4][0], hodesc[1][1], hodesc[1][2], hodesc[1][3])], fn=hd.lib.pbd_augment_frames) == -1
    assert call(descs=hdesc, odesc=hodesc, jobs=[jobs[0], (9, False, 1.0)], fn=hd.lib.pbd_augment_frames) == -1
    nanf = [np.array(f) for f in AC.frames(np.float32, 3)]
    nanf[2][1, 1, 1] = np.nan
    ndesc = [(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in nanf]
    assert call(descs=ndesc, code=5, odesc=hodesc, fn=hd.lib.pbd_augment_frames) == -1 and "frame 2" in hd.lib.pbd_last_error(hd.h).decode()
    assert hd.lib.pbd_augment_frames_device(hd.h, 6, None, 3, 0, 2, _lib.augment_array(jobs), _lib.frame_array(odesc)) == -1
    assert hd.lib.pbd_augment_frames_device(hd.h, 6, _lib.frame_array(descs), 3, 0, 2, None, _lib.frame_array(odesc)) == -1
    assert hd.lib.pbd_augment_frames_device(hd.h, 6, _lib.frame_array(descs), 3, 0, 2, _lib.augment_array(jobs), None) == -1
    # njobs == 0 is fine, with or without arrays
    assert call(njobs=0) == 0 and hd.lib.pbd_augment_frames_device(hd.h, 0, None, 3, 0, 0, None, None) == 0
    # nothing was written, and the resident result is the detect call's
    torch.cuda.synchronize()
    assert all((b.cpu().numpy() == SENTINEL).all() for b in bufs) and all((o == SENTINEL).all() for o in host_out)
    ex_after = hd.examples(before[:4])
    assert ex_after[0].tobytes() == ex_before[0].tobytes() and ex_after[1].tobytes() == ex_before[1].tobytes()
    # the same call, unedited, is taken -- and still leaves the resident result and the detect path alone
    assert call() == 0
    hd.check(hd.lib.pbd_synchronize(hd.h))
    check_destinations(bufs, reference(np.uint8, 3, tuple(jobs)))
    ex_after = hd.examples(before[:4])
    assert ex_after[0].tobytes() == ex_before[0].tobytes() and ex_after[1].tobytes() == ex_before[1].tobytes()
    assert records(hd, scene).tobytes() == before.tobytes()


def test_refused_while_a_batch_is_in_flight():
    import torch
    det = detector.PartsBasedDetector(max_batch=2)
    det.distributeModel(M.synthetic_tiny_model(thresh=-1e9))
    try:
        fr = AC.frames(np.uint8, 3)
        d_fr = upload(fr[:2])
        descs = [(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)) for t in d_fr]
        bufs, odesc = padded_destinations([(2, 3)], 1, 3)
        args = (det.hd.h, 2, _lib.frame_array(descs), 3, 0, 1, _lib.augment_array([(1, True, 0.0)]), _lib.frame_array(odesc))
        det.submit_batch([synth.synthetic_frame(5, 64, 72)])
        assert det.hd.lib.pbd_augment_frames_device(*args) == -5
        host = np.zeros((2, 3, 3), np.uint8)
        hargs = (det.hd.h, 2, _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr[:2]]), 3, 0, 1,
                 _lib.augment_array([(1, True, 0.0)]), _lib.frame_array([(host.ctypes.data, 2, 3, 9)]))
        assert det.hd.lib.pbd_augment_frames(*hargs) == -5
        got = det.wait_batch()
        torch.cuda.synchronize()
        assert (bufs[0].cpu().numpy() == SENTINEL).all() and not host.any() and len(got) > 0
        assert det.hd.lib.pbd_augment_frames_device(*args) == 0
        det.hd.check(det.hd.lib.pbd_synchronize(det.hd.h))
        check_destinations(bufs, [fr[1][:, ::-1]])
    finally:
        det.hd.close()
