"""Suppression of a caller's list on the device (pbd_suppress, pbd_suppress_device; Handle.suppress, PartsBasedDetector.suppress)
and the chain detect(im, depth) runs with setDepthConsistency on.  pbd_suppress is the pbd_set_nms stage: on an unsuppressed list
it must return exactly what pbd_set_nms returns for the same batch -- for equal and mixed sizes, and for the merged lists of
level-sharded handles, where pbd_set_nms itself is refused."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, consistency, detector, synth
from partsbaseddetector_amd import model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def model():
    return M.synthetic_person_model()


@pytest.fixture(scope="module")
def hd(model):
    h = detector.Handle(model, device=0, max_batch=8)
    yield h
    h.close()


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def raw_frames(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, 3, 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def device_suppress(hd, shapes, overlap, rec, frame_offset=0):
    import torch
    pay = torch.zeros(1 + len(rec) * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = len(rec)
    pay[1:] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
    out = torch.full((1 + len(rec) * hd.stride,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.suppress_device(shapes, overlap, pay.data_ptr(), len(rec), frame_offset, out.data_ptr(), len(rec))
    hd.check(hd.lib.pbd_synchronize(hd.h))
    n = int(out[0].item())
    return out[1:1 + max(n, 0) * hd.stride].cpu().numpy().reshape(-1, hd.stride), n


@pytest.mark.parametrize("overlap", [0.1, 0.5])
def test_equal_sizes_match_set_nms(hd, overlap):
    frames = [synth.synthetic_frame(s) for s in (1, 2, 3)]
    hd.set_nms(None)
    raw = raw_batch(hd, frames)
    hd.set_nms(overlap)
    want = raw_batch(hd, frames)
    hd.set_nms(None)
    assert 0 < len(want) < len(raw)
    shapes = [(480, 640)] * 3
    assert np.array_equal(hd.suppress(shapes, overlap, raw), want)
    got, n = device_suppress(hd, shapes, overlap, raw)
    assert n == len(want) and np.array_equal(got, want)
    # a frame offset: the frame fields stay as they are
    off = raw.copy()
    off[:, 0] += 9
    want9 = want.copy()
    want9[:, 0] += 9
    assert np.array_equal(hd.suppress(shapes, overlap, off, frame_offset=9), want9)
    got, n = device_suppress(hd, shapes, overlap, off, 9)
    assert np.array_equal(got, want9)


def test_mixed_sizes_match_set_nms(hd):
    frames = [synth.synthetic_frame(4, 480, 640), synth.synthetic_frame(5, 300, 420), synth.synthetic_frame(6, 720, 1280)]
    hd.set_nms(None)
    raw = raw_frames(hd, frames)
    hd.set_nms(0.1)
    want = raw_frames(hd, frames)
    hd.set_nms(None)
    shapes = [f.shape[:2] for f in frames]
    assert np.array_equal(hd.suppress(shapes, 0.1, raw), want)
    got, n = device_suppress(hd, shapes, 0.1, raw)
    assert np.array_equal(got, want)


def test_device_list_checks(hd):
    frames = [synth.synthetic_frame(7)]
    raw = raw_batch(hd, frames)
    bad = raw.copy()
    bad[len(bad) // 2, 0] = 3                          # frame out of range
    got, n = device_suppress(hd, [(480, 640)], 0.1, bad)
    assert n == -1 and len(got) == 0
    rc = hd.lib.pbd_suppress(hd.h, 1, _lib.ptr(np.array([480], np.int32), C.c_int), _lib.ptr(np.array([640], np.int32), C.c_int), 0.1,
                             bad.ctypes.data, len(bad), 0, bad.ctypes.data, len(bad), C.byref(C.c_int()))
    assert rc == -1 and f"record {len(bad) // 2}" in hd.lib.pbd_last_error(hd.h).decode()


def test_device_overflowed_or_truncated_input_gives_minus_one(hd):
    import torch
    raw = raw_batch(hd, [synth.synthetic_frame(10)])
    n = len(raw)
    pay = torch.zeros(1 + n * hd.stride, dtype=torch.int32, device="cuda")
    pay[1:] = torch.from_numpy(raw.ravel()).cuda()
    out = torch.full((1 + n * hd.stride,), -7, dtype=torch.int32, device="cuda")
    for word0 in (-1, n + 1):
        pay[0] = word0
        out.fill_(-7)
        torch.cuda.synchronize()
        hd.suppress_device([(480, 640)], 0.1, pay.data_ptr(), n, 0, out.data_ptr(), n)
        hd.check(hd.lib.pbd_synchronize(hd.h))
        o = out.cpu().numpy()
        assert o[0] == -1 and (o[1:] == -7).all(), word0
    # capacity 0 is refused (pbd.h)
    ir, ic = np.array([480], np.int32), np.array([640], np.int32)
    rc = hd.lib.pbd_suppress_device(hd.h, 1, _lib.ptr(ir, C.c_int), _lib.ptr(ic, C.c_int), 0.1, pay.data_ptr(), 0, 0, out.data_ptr(), n)
    assert rc == -1 and "capacity 0" in hd.lib.pbd_last_error(hd.h).decode()


def test_level_sharding_union(model):
    frame = synth.synthetic_frame(8)
    full = detector.Handle(model, device=0)
    full.set_nms(0.1)
    want = raw_batch(full, [frame])
    full.close()
    ranks = []
    lists = []
    for r in range(2):
        h = detector.Handle(model, device=0)
        h.set_level_shard(r, 2)
        lists.append(raw_batch(h, [frame]))
        ranks.append(h)
    merged = np.concatenate(lists)
    order = np.lexsort((merged[:, 3], merged[:, 4], merged[:, 1], merged[:, 2]))   # (level, component, root_y, root_x)
    merged = merged[order]
    got = ranks[0].suppress([(480, 640)], 0.1, merged)
    assert np.array_equal(got, want)
    got, n = device_suppress(ranks[1], [(480, 640)], 0.1, merged)
    assert np.array_equal(got, want)
    for h in ranks:
        h.close()


def mirror_suppress(hd, rec, shape, overlap):
    cands = hd.unpack_candidates(np.ascontiguousarray(rec).ravel(), len(rec))
    for c, r in zip(cands, rec):
        c._rec = r
    detector.Candidate.sort(cands)
    detector.Candidate.nonMaximaSuppression(shape, cands, overlap)
    return np.array([c._rec for c in cands], np.int32).reshape(-1, hd.stride)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_detect_with_depth_chain(model, dtype):
    det = detector.PartsBasedDetector(nms=0.1, dtype=dtype)
    det.distributeModel(model)
    frame = synth.synthetic_frame(9)
    d = synth.synthetic_depth(80, 480, 640, dtype=np.float32)
    det.hd.set_nms(None)
    raw = raw_batch(det.hd, [frame])
    det.hd.set_nms(0.1)
    plain = det.hd.pack_candidates(det.detect(frame, d))
    det.setDepthConsistency(0.03)
    got = det.hd.pack_candidates(det.detect(frame, d))
    filt = consistency.filter_records(det.hd.flat, raw, [d], 0.03, dtype)
    want = mirror_suppress(det.hd, filt, (480, 640), 0.1)
    want = det.hd.pack_candidates(det.hd.unpack_candidates(want.ravel(), len(want)))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, plain)
    assert det.hd.nms_overlap == 0.1                    # the handle's own setting is back
    det.setDepthConsistency(None)
    assert np.array_equal(det.hd.pack_candidates(det.detect(frame, d)), plain)
    det.hd.close()
