"""Depth consistency of candidate records on the device (pbd_depth_consistency, pbd_depth_consistency_device; Handle.depth_consistency,
PartsBasedDetector.filterCandidatesByDepth).  The yardstick is consistency.filter_records, the numpy mirror of
SearchSpacePruning<T>::filterCandidatesByDepth with the project's decisions (tests/test_depth_consistency_cpu.py pins it against a
literal transcription).  Every comparison is of the kept records' int32 words and their order."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, consistency, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu
DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def model():
    return M.synthetic_person_model()


@pytest.fixture(scope="module")
def handles(model):
    hs = {rt: detector.Handle(model, device=0, max_batch=8, real_type=rt) for rt in (_lib.REAL_F32, _lib.REAL_F64)}
    yield hs
    for h in hs.values():
        h.close()


def T_of(hd):
    return np.float32 if hd.dtype == np.float32 else np.float64


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def record(hd, frame, parts, component=0):
    r = np.zeros(hd.stride, np.int32)
    parts = np.asarray(parts, np.int32).reshape(-1, 4)
    r[0], r[1], r[6] = frame, component, len(parts)
    r[8:8 + parts.size] = parts.ravel()
    return r


def check(hd, depths, rec, z, frame_offset=0):
    got = hd.depth_consistency(depths, rec, z, frame_offset)
    want = consistency.filter_records(hd.flat, rec, depths, z, T_of(hd), frame_offset)
    assert got.shape == want.shape and np.array_equal(got, want), (len(got), len(want))
    return got


def scaled_depth(seed, rows, cols, dtype):
    d = synth.synthetic_depth(seed, rows, cols, dtype=np.float64 if dtype in (np.float32, np.float64) else np.uint16)
    if dtype == np.uint8:
        d = (d // 16).astype(np.uint8)
    return d.astype(dtype)


@pytest.fixture(scope="module")
def person_lists(handles):
    frames = [synth.synthetic_frame(s) for s in (1, 2)]
    return frames, {rt: raw_batch(hd, frames) for rt, hd in handles.items()}


# ---- the person model on synthetic frames, every depth code, both real types ----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [_lib.REAL_F32, _lib.REAL_F64])
def test_person_every_code(handles, person_lists, rt, dtype):
    hd = handles[rt]
    rec = person_lists[1][rt]
    assert len(rec) > 50
    depths = [scaled_depth(10 + f, 480, 640, dtype) for f in range(2)]
    ints = dtype in (np.uint8, np.uint16)
    nkept = []
    for z in ((0.03, 20.0, 200.0) if ints else (0.03, 0.3)):
        nkept.append(len(check(hd, depths, rec, z)))
    assert any(0 < k < len(rec) for k in nkept), nkept


def test_float_and_double_disagree(handles):
    hd32, hd64 = handles[_lib.REAL_F32], handles[_lib.REAL_F64]
    flat = hd32.flat
    norm = consistency.anchor_norms(flat)
    thr = norm[1] * float(np.float32(0.03))
    a = 1.0
    for k in range(-400, 400):
        b = a + thr + k * 2.0 ** -40
        if (float(abs(np.float32(b) - np.float32(a))) > thr) != (abs(b - a) > thr):
            break
    d = np.full((40, 40), a, np.float64)
    d[:, 20:] = b
    parts = [[0, 0, 10, 10]] * 26
    parts[1] = [25, 5, 10, 10]
    rec = record(hd32, 0, parts)[None]
    got32 = check(hd32, [d], rec, 0.03)
    got64 = check(hd64, [d], rec, 0.03)
    assert len(got32) != len(got64)


@pytest.mark.parametrize("rt", [_lib.REAL_F32, _lib.REAL_F64])
def test_boxes_partly_and_fully_outside(handles, rt):
    hd = handles[rt]
    rng = np.random.default_rng(3)
    d = scaled_depth(4, 120, 160, np.float32)
    recs = []
    for i in range(400):
        parts = [[int(rng.integers(-60, 200)), int(rng.integers(-60, 160)), int(rng.integers(0, 70)), int(rng.integers(0, 70))]
                 for _ in range(26)]
        recs.append(record(hd, 0, parts))
    recs.append(record(hd, 0, [[-1000, -1000, 5, 5]] * 26))
    recs.append(record(hd, 0, [[2 ** 31 - 10, 2 ** 31 - 10, 100, 100]] * 26))
    recs = np.stack(recs)
    for z in (0.03, 0.3, 3.0):
        check(hd, [d], recs, z)


@pytest.mark.parametrize("rt", [_lib.REAL_F32, _lib.REAL_F64])
def test_1080p_large_boxes(handles, rt):
    hd = handles[rt]
    frame = synth.synthetic_frame(21, 1080, 1920)
    rec = raw_batch(hd, [frame])
    areas = (rec[:, 10::4][:, :26].astype(np.int64) * rec[:, 11::4][:, :26]).max(axis=1)
    big = np.argsort(-areas, kind="stable")[:300]
    sel = rec[np.sort(big)]
    assert areas.max() > 4096                         # the streaming class runs
    for dtype in (np.uint16, np.float64):
        d = scaled_depth(22, 1080, 1920, dtype)
        check(hd, [d], sel, 0.03 if dtype == np.float64 else 20.0)


def test_ten_thousand_records(handles):
    hd = handles[_lib.REAL_F32]
    rng = np.random.default_rng(11)
    d = [scaled_depth(30 + f, 480, 640, np.float32) for f in range(2)]
    n = 10240
    # the parts of a record near one spot (mostly one surface), boxes of every size class
    x = rng.integers(-20, 640, (n, 1)) + rng.integers(-15, 16, (n, 26))
    y = rng.integers(-20, 480, (n, 1)) + rng.integers(-15, 16, (n, 26))
    s = rng.choice([1, 4, 12, 30, 70], (n, 26))
    parts = np.stack([x, y, s, s], axis=2)
    rec = np.zeros((n, hd.stride), np.int32)
    rec[:, 0] = np.arange(n) % 2
    rec[:, 6] = 26
    rec[:, 8:8 + 26 * 4] = parts.reshape(n, -1)
    kept = [len(check(hd, d, rec, z)) for z in (0.3, 3.0)]
    assert any(0 < k < n for k in kept), kept


@pytest.mark.parametrize("rt", [_lib.REAL_F32, _lib.REAL_F64])
def test_more_than_sixteen_thousand_records_host_and_device(handles, rt):
    """lists longer than 64 compaction workgroups of 256 records: every kept record counted, in both forms"""
    import torch
    hd = handles[rt]
    rng = np.random.default_rng(17)
    d = [scaled_depth(90 + f, 480, 640, np.float32) for f in range(2)]
    n = 20480
    x = rng.integers(-20, 640, (n, 1)) + rng.integers(-15, 16, (n, 26))
    y = rng.integers(-20, 480, (n, 1)) + rng.integers(-15, 16, (n, 26))
    s = rng.choice([1, 4, 12, 30, 70], (n, 26))
    rec = np.zeros((n, hd.stride), np.int32)
    rec[:, 0] = np.arange(n) % 2
    rec[:, 6] = 26
    rec[:, 8:8 + 26 * 4] = np.stack([x, y, s, s], axis=2).reshape(n, -1)
    want = consistency.filter_records(hd.flat, rec, d, 0.3, T_of(hd))
    assert 16384 < len(want) < n                    # kept records past the 64th compaction workgroup
    got = hd.depth_consistency(d, rec, 0.3)
    assert got.shape == want.shape and np.array_equal(got, want)
    dev = torch.device("cuda", 0)
    dd = [torch.from_numpy(x).to(dev) for x in d]
    pay = torch.zeros(1 + n * hd.stride, dtype=torch.int32, device=dev)
    pay[0] = n
    pay[1:] = torch.from_numpy(rec.ravel()).to(dev)
    out = torch.full((1 + n * hd.stride,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hd.depth_consistency_device([(t.data_ptr(), 480, 640, 640 * 4) for t in dd], 5, 0.3, pay.data_ptr(), n, 0, out.data_ptr(), n)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    o = out.cpu().numpy()
    assert o[0] == len(want)
    assert np.array_equal(o[1:1 + len(want) * hd.stride].reshape(-1, hd.stride), want)


def test_one_part_component_keeps():
    hd = detector.Handle(M.synthetic_model(seed=5, pa=[0], nmix=1, name="one"), device=0)
    try:
        d = np.arange(100, dtype=np.float32).reshape(10, 10)
        rec = np.stack([record(hd, 0, [[0, 0, 3, 3]]), record(hd, 0, [[50, 50, 3, 3]])])
        assert np.array_equal(hd.depth_consistency([d], rec, 0.03), rec)
    finally:
        hd.close()


# ---- the device form after pbd_detect_batch_device_out with a frame offset --------------------------------------------------------
@pytest.mark.parametrize("rt", [_lib.REAL_F32, _lib.REAL_F64])
def test_device_after_detect_batch_device_out(handles, person_lists, rt):
    import torch
    hd = handles[rt]
    frames = person_lists[0]
    dev = torch.device("cuda", 0)
    d_frames = torch.from_numpy(np.stack(frames)).to(dev)
    depths = [scaled_depth(40 + f, 480, 640, np.float32) for f in range(2)]
    # a region of a larger device image, read in place
    big = torch.zeros((2, 500, 700), dtype=torch.float32, device=dev)
    for f in range(2):
        big[f, 10:490, 30:670] = torch.from_numpy(depths[f]).to(dev)
    torch.cuda.synchronize()
    cap = hd.max_candidates
    pay = torch.full((1 + cap * hd.stride,), -7, dtype=torch.int32, device=dev)
    out = torch.full((1 + cap * hd.stride,), -7, dtype=torch.int32, device=dev)
    hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, 2, d_frames.data_ptr(), 480, 640, 3, 5, pay.data_ptr(), cap))
    descs = [(big[f, 10, 30:].data_ptr(), 480, 640, 700 * 4) for f in range(2)]
    hd.depth_consistency_device(descs, 5, 0.3, pay.data_ptr(), cap, 5, out.data_ptr(), cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    n_in = int(pay[0].item())
    rec = pay[1:1 + n_in * hd.stride].cpu().numpy().reshape(n_in, hd.stride)
    assert np.array_equal(rec[:, 0] >= 5, np.ones(n_in, bool))
    n = int(out[0].item())
    got = out[1:1 + n * hd.stride].cpu().numpy().reshape(n, hd.stride)
    want = consistency.filter_records(hd.flat, rec, depths, 0.3, T_of(hd), 5)
    assert np.array_equal(got, want)
    assert 0 < n < n_in


def test_device_overflow_and_truncation(handles):
    import torch
    hd = handles[_lib.REAL_F32]
    dev = torch.device("cuda", 0)
    d = scaled_depth(50, 64, 64, np.float32)
    rng = np.random.default_rng(5)
    rec = np.stack([record(hd, 0, rng.integers(0, 40, (26, 4))) for _ in range(40)])
    want = consistency.filter_records(hd.flat, rec, [d], 0.3, np.float32)
    assert 3 < len(want)
    d_depth = torch.from_numpy(d).to(dev)
    pay = torch.zeros(1 + 40 * hd.stride, dtype=torch.int32, device=dev)
    pay[1:] = torch.from_numpy(rec.ravel()).to(dev)
    out = torch.full((1 + 40 * hd.stride,), -7, dtype=torch.int32, device=dev)
    descs = [(d_depth.data_ptr(), 64, 64, 256)]

    def run(word0, capacity, out_cap):
        pay[0] = word0
        out.fill_(-7)
        torch.cuda.synchronize()
        hd.depth_consistency_device(descs, 5, 0.3, pay.data_ptr(), capacity, 0, out.data_ptr(), out_cap)
        hd.check(hd.lib.pbd_synchronize(hd.h))
        return out.cpu().numpy()

    o = run(40, 40, 40)
    assert o[0] == len(want) and np.array_equal(o[1:1 + len(want) * hd.stride].reshape(-1, hd.stride), want)
    o = run(-1, 40, 40)
    assert o[0] == -1 and (o[1:] == -7).all()
    o = run(41, 40, 40)
    assert o[0] == -1 and (o[1:] == -7).all()
    o = run(40, 40, 2)                                  # truncated output: word 0 is still the kept count
    assert o[0] == len(want) and np.array_equal(o[1:1 + 2 * hd.stride].reshape(-1, hd.stride), want[:2])
    assert (o[1 + 2 * hd.stride:] == -7).all()
    # the host form: capacity below the kept count
    got = np.zeros((2, hd.stride), np.int32)
    n = C.c_int()
    rc = hd.lib.pbd_depth_consistency(hd.h, 1, _lib.frame_array([(d.ctypes.data, 64, 64, 256)]), 5, 0.3, rec.ctypes.data, 40, 0,
                                      got.ctypes.data, 2, C.byref(n))
    assert rc == -4 and n.value == len(want) and np.array_equal(got, want[:2])
    # in place
    inplace = rec.copy()
    rc = hd.lib.pbd_depth_consistency(hd.h, 1, _lib.frame_array([(d.ctypes.data, 64, 64, 256)]), 5, 0.3, inplace.ctypes.data, 40, 0,
                                      inplace.ctypes.data, 40, C.byref(n))
    assert rc == 0 and np.array_equal(inplace[:n.value], want)


def test_refusals_name_the_index_and_leave_the_resident_result(handles, person_lists):
    import torch
    hd = handles[_lib.REAL_F32]
    frames = person_lists[0]
    raw = raw_batch(hd, frames)
    before = hd.get_stage(_lib.STAGE_ROOTV, 1, 3, *hd.plan(480, 640)["feat_rows"][3:4], hd.plan(480, 640)["feat_cols"][3])
    d = scaled_depth(60, 480, 640, np.float32)
    good = (d.ctypes.data, 480, 640, d.strides[0])
    lib, n = hd.lib, C.c_int()
    out = np.zeros_like(raw)

    def host(descs, code, z, rec, msg):
        rc = lib.pbd_depth_consistency(hd.h, len(descs), _lib.frame_array(descs), code, z, rec.ctypes.data, len(rec), 0,
                                       out.ctypes.data, len(out), C.byref(n))
        assert rc == -1, rc
        assert msg in lib.pbd_last_error(hd.h).decode(), lib.pbd_last_error(hd.h)

    host([good, good], 3, 0.03, raw, "depth code 3")
    host([good, (d.ctypes.data, 0, 640, d.strides[0])], 5, 0.03, raw, "frame 1")
    host([good, (d.ctypes.data, 480, 640, 100)], 5, 0.03, raw, "frame 1: stride")
    host([good, good], 5, float("nan"), raw, "zfactor")
    bad = raw.copy()
    bad[7, 0] = 2
    host([good, good], 5, 0.03, bad, "record 7")
    bad = raw.copy()
    bad[9, 6] = 25
    host([good, good], 5, 0.03, bad, "record 9")
    dt = torch.from_numpy(d).cuda()
    pay = torch.zeros(1 + 4 * hd.stride, dtype=torch.int32, device="cuda")
    rc = lib.pbd_depth_consistency_device(hd.h, 2, _lib.frame_array([(dt.data_ptr(), 480, 640, 2560), (dt.data_ptr() + 2, 480, 640, 2560)]),
                                          5, 0.03, pay.data_ptr(), 4, 0, pay.data_ptr(), 4)
    assert rc == -1 and "frame 1" in lib.pbd_last_error(hd.h).decode()
    after = hd.get_stage(_lib.STAGE_ROOTV, 1, 3, *hd.plan(480, 640)["feat_rows"][3:4], hd.plan(480, 640)["feat_cols"][3])
    assert np.array_equal(before, after)
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    # the resident list re-emitted after all of the above
    pay2 = torch.zeros(1 + len(raw) * hd.stride, dtype=torch.int32, device="cuda")
    hd.check(lib.pbd_argmin_device_out(hd.h, 0, pay2.data_ptr(), len(raw)))
    hd.check(lib.pbd_synchronize(hd.h))
    assert np.array_equal(pay2[1:].cpu().numpy().reshape(-1, hd.stride), raw)
    del buf


def test_filterCandidatesByDepth(model):
    det = detector.PartsBasedDetector()
    det.distributeModel(model)
    frame = synth.synthetic_frame(3)
    cands = det.detect(frame)
    d = scaled_depth(70, 480, 640, np.float32)
    kept = det.filterCandidatesByDepth(cands, d, 0.3)
    want = consistency.filter_records(det.hd.flat, det.hd.pack_candidates(cands), [d], 0.3, np.float32)
    assert np.array_equal(det.hd.pack_candidates(kept), want)
    assert 0 < len(kept) < len(cands)
    # depth is ignored unless the setting is on
    assert det.hd.pack_candidates(det.detect(frame, d)).tobytes() == det.hd.pack_candidates(cands).tobytes()
    det.setDepthConsistency(0.3)
    assert np.array_equal(det.hd.pack_candidates(det.detect(frame, d)), want)
    assert det.hd.pack_candidates(det.detect(frame, None)).tobytes() == det.hd.pack_candidates(cands).tobytes()
    det.hd.close()
