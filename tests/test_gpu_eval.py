"""Testing a model on the device: pbd_part_nms, pbd_best_overlap, pbd_eval_pck, pbd_eval_apk (host and _device forms) and the
drivers PartsBasedDetector.testModel / testModelGtbox against the numpy yardstick (partsbaseddetector_amd/evaluation.py), byte
for byte, on the built cases of tests/eval_hard_cases.py."""
import ctypes as C

import numpy as np
import pytest

import eval_hard_cases as H
from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import evaluation as ev
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

OFF = 7      # the frame offset the calls are exercised with


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def handles():
    hs = {1: detector.Handle(H.model1(), device=0), 2: detector.Handle(H.model2(), device=0, max_batch=2),
          26: detector.Handle(H.model26(), device=0)}
    for n, h in hs.items():
        assert h.eval_nparts() == n and h.stride == 8 + 4 * n
    yield hs
    for h in hs.values():
        h.close()


def payload(rec, stride, word0=None, cap=None):
    import torch
    cap = len(rec) if cap is None else cap
    pay = torch.zeros(1 + max(cap, 1) * stride, dtype=torch.int32, device="cuda")
    pay[0] = len(rec) if word0 is None else word0
    if len(rec):
        pay[1:1 + rec.size] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
    return pay


def device_nms(hd, nframes, overlap, max_boxes, rec, frame_offset=0, word0=None, out_cap=None):
    import torch
    pay = payload(rec, hd.stride, word0)
    out_cap = len(rec) if out_cap is None else out_cap
    out = torch.full((1 + max(len(rec), 1) * hd.stride,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.part_nms_device(nframes, overlap, max_boxes, pay.data_ptr(), len(rec), frame_offset, out.data_ptr(), out_cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    o = out.cpu().numpy()
    n = int(o[0])
    m = min(max(n, 0), out_cap)
    assert (o[1 + m * hd.stride:] == -7).all()                       # nothing past the kept records is written
    return o[1:1 + m * hd.stride].reshape(-1, hd.stride), n


def device_best(hd, gt, overlap, rec, frame_offset=0):
    import torch
    pay = payload(rec, hd.stride)
    out = torch.full((len(gt) * (hd.stride + 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.best_overlap_device(gt, overlap, pay.data_ptr(), len(rec), frame_offset, out.data_ptr(), out.data_ptr() + 4 * len(gt) * hd.stride)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    o = out.cpu().numpy()
    return o[:len(gt) * hd.stride].reshape(len(gt), hd.stride), o[len(gt) * hd.stride:]


def device_pck(hd, rec, found, gt, scale, thresh):
    import torch
    n, npart = len(rec), hd.eval_nparts()
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
    d_found = torch.from_numpy(np.ascontiguousarray(found, np.int32)).cuda()
    out = torch.full((npart * (n + 1),), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hd.eval_pck_device(n, d_rec.data_ptr(), d_found.data_ptr(), gt, scale, thresh, out.data_ptr(), out.data_ptr() + 8 * npart)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    o = out.cpu().numpy()
    return o[:npart], o[npart:].reshape(npart, n)


def device_apk(hd, rec, gt_offset, gt, gs, thresh, frame_offset=0, word0=None):
    import torch
    n, npart = len(rec), hd.eval_nparts()
    pay = payload(rec, hd.stride, word0)
    out = torch.full((npart * (2 * n + 1),), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    base = out.data_ptr()
    hd.eval_apk_device(gt_offset, gt, gs, thresh, pay.data_ptr(), n, frame_offset, base, base + 8 * npart, base + 8 * npart * (n + 1),
                       status.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    o = out.cpu().numpy()
    return o[:npart], o[npart:npart * (n + 1)].reshape(npart, n), o[npart * (n + 1):].reshape(npart, n), int(status.item())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- part NMS ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 2, 26])
def test_nms_built_cases(handles, nparts):
    hd = handles[nparts]
    for name, overlap, max_boxes, rows, kept in H.nms_cases(nparts):
        rec = H.records(nparts, rows)
        want = ev.nms_frame(rec, nparts, overlap, max_boxes)
        assert same(want, rec[kept])
        assert same(hd.part_nms(1, overlap, rec, max_boxes), want), name
        got, n = device_nms(hd, 1, overlap, max_boxes, rec)
        assert n == len(want) and same(got, want), name


_many = {}


def many_frames(max_boxes):
    if max_boxes not in _many:
        rec, nframes = H.nms_many_frames(2, frame_offset=OFF)
        _many[max_boxes] = (rec, nframes, ev.part_nms(rec, nframes, 2, 0.3, max_boxes, frame_offset=OFF))
    return _many[max_boxes]


@pytest.mark.parametrize("max_boxes", [5, 1000])
def test_nms_frames_of_every_size_in_one_call(handles, max_boxes):
    hd = handles[2]
    rec, nframes, want = many_frames(max_boxes)
    assert 0 < len(want) < len(rec) and len(np.unique(want[:, 0])) == sum(1 for c in H.NMS_FRAME_COUNTS if c)
    assert same(hd.part_nms(nframes, 0.3, rec, max_boxes, frame_offset=OFF), want)
    got, n = device_nms(hd, nframes, 0.3, max_boxes, rec, frame_offset=OFF)
    assert n == len(want) and same(got, want)
    # a short output: the count is the whole count, the first records are written
    got, n = device_nms(hd, nframes, 0.3, max_boxes, rec, frame_offset=OFF, out_cap=3)
    assert n == len(want) and same(got, want[:3])
    with pytest.raises(PbdError) as e:
        hd.part_nms(nframes, 0.3, rec, max_boxes, frame_offset=OFF, capacity=3)
    assert e.value.code == -4


def test_nms_26_parts(handles):
    hd = handles[26]
    rec = np.concatenate([H.random_records(31, 300, 26, 0, span=250, nan=1), H.random_records(32, 70, 26, 1, span=100)])
    want = ev.part_nms(rec, 2, 26, 0.3)
    assert 0 < len(want) < len(rec)
    assert same(hd.part_nms(2, 0.3, rec), want)
    got, n = device_nms(hd, 2, 0.3, 1000, rec)
    assert n == len(want) and same(got, want)


def test_nms_select_of_70000_records(handles):
    hd = handles[2]
    rec = H.random_records(41, 70000, 2, 0, span=3000, nan=3)
    sc = np.sort(ev.scores(rec)[~np.isnan(ev.scores(rec))])[::-1]
    assert sc[999] == sc[1000], "equal scores straddle the cut"
    want = ev.part_nms(rec, 1, 2, 0.3)
    assert 100 < len(want) < 1000
    got, n = device_nms(hd, 1, 0.3, 1000, rec)
    assert n == len(want) and same(got, want)
    assert same(hd.part_nms(1, 0.3, rec, 17), ev.part_nms(rec, 1, 2, 0.3, 17))


def test_nms_refusals(handles):
    hd = handles[2]
    rec = H.random_records(51, 20, 2, 0)
    for bad in (0, 1001, -1):
        with pytest.raises(PbdError) as e:
            hd.part_nms(1, 0.3, rec, bad)
        assert e.value.code == -1 and "max_boxes" in str(e.value)
    for kw in (dict(overlap=float("nan")), dict(nframes=0)):
        with pytest.raises(PbdError) as e:
            hd.part_nms(kw.get("nframes", 1), kw.get("overlap", 0.3), rec)
        assert e.value.code == -1
    with pytest.raises(PbdError) as e:
        hd.part_nms_device(1, float("nan"), 1000, 0, 0, 0, 0, 0)
    assert e.value.code == -1
    # host records: a frame out of range, below its predecessor's, a bad part count
    for row, col, val in ((5, 0, 1), (0, 0, -1), (7, 6, 3)):
        bad = rec.copy()
        bad[row, col] = val
        with pytest.raises(PbdError) as e:
            hd.part_nms(1, 0.3, bad)
        assert e.value.code == -1 and f"record {row}" in str(e.value)
    two = rec.copy()
    two[:10, 0] = 1                                                   # frame 1 before frame 0
    with pytest.raises(PbdError) as e:
        hd.part_nms(2, 0.3, two)
    assert e.value.code == -1 and "record 10" in str(e.value)
    # the device form: word 0 = -1 and nothing else written
    for kw in (dict(word0=-1), dict(word0=len(rec) + 1)):
        got, n = device_nms(hd, 1, 0.3, 1000, rec, **kw)
        assert n == -1 and len(got) == 0
    got, n = device_nms(hd, 2, 0.3, 1000, two)
    assert n == -1
    oor = rec.copy()
    oor[3, 0] = 1
    got, n = device_nms(hd, 1, 0.3, 1000, oor)
    assert n == -1
    # an empty list
    assert len(hd.part_nms(3, 0.3, rec[:0])) == 0
    got, n = device_nms(hd, 3, 0.3, 1000, rec[:0])
    assert n == 0
    # components of different part counts
    m = M.synthetic_tiny_model()
    m.filterid.append([list(x) for x in m.filterid[0][:2]])
    m.biasid.append([list(x) for x in m.biasid[0][:2]])
    m.defid.append([list(x) for x in m.defid[0][:2]])
    m.parentid.append(list(m.parentid[0][:2]))
    mixed = detector.Handle(m, device=0)
    try:
        r3 = H.random_records(52, 4, 3, 0)
        for call in (lambda: mixed.part_nms(1, 0.3, r3), lambda: mixed.best_overlap([[0, 0, 9, 9]], 0.3, r3),
                     lambda: mixed.eval_apk(r3, [0, 1], np.zeros((1, 3, 2)), [1.0])):
            with pytest.raises(PbdError) as e:
                call()
            assert e.value.code == -2
        assert mixed.lib.pbd_eval_pck(mixed.h, 1, r3.ctypes.data, r3.ctypes.data, r3.ctypes.data, r3.ctypes.data, 0.5, r3.ctypes.data, None) == -2
    finally:
        mixed.close()


def test_refused_while_a_batch_is_in_flight(handles):
    hd = handles[2]
    ims = [np.ascontiguousarray(synth.synthetic_frame(60 + k, 48, 64)) for k in range(2)]
    rec = H.random_records(53, 10, 2, 0)
    hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 2, _lib.ptr_array(ims), 48, 64, 3, ims[0].strides[0]))
    try:
        for call in (lambda: hd.part_nms(1, 0.3, rec), lambda: hd.best_overlap([[0, 0, 9, 9]], 0.3, rec),
                     lambda: hd.eval_pck(rec[:1], [1], np.zeros((1, 2, 2)), [1.0]),
                     lambda: hd.eval_apk(rec, [0, 1], np.zeros((1, 2, 2)), [1.0])):
            with pytest.raises(PbdError) as e:
                call()
            assert e.value.code == -5
    finally:
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        hd.check(hd.lib.pbd_detect_batch_wait(hd.h, buf.ctypes.data, hd.max_candidates, C.byref(C.c_int())))


# ---- best overlap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [2, 26])
def test_best_overlap_built_cases(handles, nparts):
    hd = handles[nparts]
    rows, gt, overlap, chosen = H.best_cases(nparts)
    rec = H.records(nparts, rows)
    rec[:, 0] += OFF
    want, wfound = ev.best_overlap(rec, len(gt), nparts, gt, overlap, frame_offset=OFF)
    assert wfound.tolist() == [int(c is not None) for c in chosen]
    out, found = hd.best_overlap(gt, overlap, rec, frame_offset=OFF)
    assert same(out, want) and same(found, wfound)
    out, found = device_best(hd, gt, overlap, rec, frame_offset=OFF)
    assert same(out, want) and same(found, wfound)
    with pytest.raises(PbdError) as e:
        hd.best_overlap(gt, float("nan"), rec, frame_offset=OFF)
    assert e.value.code == -1


def test_best_overlap_of_70000_records(handles):
    hd = handles[2]
    rec = H.random_records(43, 70000, 2, 2, span=300, nan=5)
    rec[69990:, 5] = rec[5, 5] = np.float32(9.5).view(np.int32)      # the best score at both ends of the list, on passing records
    rec[69990:, 8:] = rec[5, 8:] = [99, 99, 2, 2, 139, 149, 2, 2]
    gt = np.array([[0, 0, 50, 50], [np.nan] * 4, [100, 100, 140, 150], [0, 0, 9, 9]], np.float64)
    want, wfound = ev.best_overlap(rec, 4, 2, gt, 0.3)
    assert wfound.tolist() == [0, 0, 1, 0]
    assert same(want[2], rec[5])
    out, found = device_best(hd, gt, 0.3, rec)
    assert same(out, want) and same(found, wfound)
    out, found = hd.best_overlap(gt, 0.3, rec)
    assert same(out, want) and same(found, wfound)


# ---- PCK ---------------------------------------------------------------------------------------------------------------------
def test_pck_built_case(handles):
    hd = handles[2]
    rows, found, gt, scale, thresh, pck = H.pck_case(2)
    rec = H.records(2, rows)
    want, wdist = ev.eval_pck(rec, found, 2, gt, scale, thresh)
    assert want.tolist() == pck.tolist()
    got, dist = hd.eval_pck(rec, found, gt, scale, thresh)
    assert same(got, want) and same(dist, wdist)
    got, dist = device_pck(hd, rec, found, gt, scale, thresh)
    assert same(got, want) and same(dist, wdist)
    assert same(hd.eval_pck(rec, found, gt, scale, thresh, want_dist=False)[0], want)


@pytest.mark.parametrize("nparts,nframes", [(2, 1), (26, 300)])
def test_pck_random(handles, nparts, nframes):
    hd = handles[nparts]
    rec = H.random_records(44, nframes, nparts, 0, span=100)
    found = (synth.randint(44, nframes, 0, 4, 20) > 0).astype(np.int32)
    gt = ev.centres(rec, nparts) + synth.randint(44, nframes * nparts * 2, -9, 9, 21).reshape(nframes, nparts, 2) * 0.5
    gt[::11, 0, 1] = np.nan
    scale = 4.0 + synth.randint(44, nframes, 0, 12, 22)
    want, wdist = ev.eval_pck(rec, found, nparts, gt, scale, 0.5)
    if nframes > 1:
        assert 0 < want.min() and want.max() < 1
    got, dist = hd.eval_pck(rec, found, gt, scale, 0.5)
    assert same(got, want) and same(dist, wdist)
    got, dist = device_pck(hd, rec, found, gt, scale, 0.5)
    assert same(got, want) and same(dist, wdist)


# ---- APK ---------------------------------------------------------------------------------------------------------------------
def check_apk(hd, nparts, rec, gt_offset, gt, gs, thresh, frame_offset=0):
    want = ev.eval_apk(rec, len(gt_offset) - 1, nparts, gt_offset, gt, gs, thresh, frame_offset=frame_offset)
    got = hd.eval_apk(rec, gt_offset, gt, gs, thresh, frame_offset=frame_offset)
    for a, b in zip(got, want):
        assert same(a, b)
    dev = device_apk(hd, rec, gt_offset, gt, gs, thresh, frame_offset=frame_offset)
    assert dev[3] == len(rec)
    for a, b in zip(dev[:3], want):
        assert same(a, b)
    return want


@pytest.mark.parametrize("case", [H.apk_case, H.apk_first_jmin_case, H.apk_sum_order_case])
@pytest.mark.parametrize("nparts", [2, 26])
def test_apk_built_cases(handles, nparts, case):
    rows, gt_offset, gt, gs, thresh, tp = case(nparts)
    rec = H.records(nparts, rows)
    apk, prec, rcl = check_apk(handles[nparts], nparts, rec, gt_offset, gt, gs, thresh)
    assert prec[0].tolist() == (np.cumsum(tp) / np.arange(1, len(tp) + 1)).tolist()
    if case is H.apk_sum_order_case:
        assert apk[0] == 0.9166666666666666
    # an empty list and a one-record list
    empty = check_apk(handles[nparts], nparts, rec[:0], gt_offset, gt, gs, thresh)
    assert not empty[0].any()
    check_apk(handles[nparts], nparts, rec[1:2], gt_offset, gt, gs, thresh)


def test_apk_5000_records_of_26_parts(handles):
    rec, gt_offset, gt, gs = H.apk_random(45, 5000, 26, frame_offset=OFF)
    rec[7, 5] = rec[4000, 5] = np.float32(np.nan).view(np.int32)
    apk, prec, rcl = check_apk(handles[26], 26, rec, gt_offset, gt, gs, 0.5, frame_offset=OFF)
    assert 0 < apk.min() and apk.max() < 1 and len(np.unique(apk)) > 20


def test_apk_refusals(handles):
    hd = handles[2]
    rows, gt_offset, gt, gs, thresh, _ = H.apk_case(2)
    rec = H.records(2, rows)
    zero = np.zeros(len(gt_offset), np.int32)
    with pytest.raises(PbdError) as e:                               # G == 0
        hd.check(hd.lib.pbd_eval_apk(hd.h, len(zero) - 1, zero.ctypes.data, gt.ctypes.data, gs.ctypes.data, 0.5, rec.ctypes.data, len(rec), 0,
                                     gt.ctypes.data, None, None))
    assert e.value.code == -1 and "0 / 0" in str(e.value)
    down = gt_offset.copy()
    down[2] = 0
    with pytest.raises(PbdError) as e:
        hd.eval_apk(rec, down, gt, gs, thresh)
    assert e.value.code == -1
    bad = rec.copy()
    bad[2, 0] = 9
    with pytest.raises(PbdError) as e:
        hd.eval_apk(bad, gt_offset, gt, gs, thresh)
    assert e.value.code == -1 and "record 2" in str(e.value)
    for word0 in (-1, len(rec) + 1):                                  # a bad count: the status, and nothing else
        apk, prec, rcl, status = device_apk(hd, rec, gt_offset, gt, gs, thresh, word0=word0)
        assert status == -1 and (apk == -7).all() and (prec == -7).all() and (rcl == -7).all()


# ---- the drivers -------------------------------------------------------------------------------------------------------------
def test_drivers_and_resident_result():
    det = detector.PartsBasedDetector(max_batch=2)
    det.distributeModel(H.model2())
    hd = det.hd
    frames = [synth.synthetic_frame(71, 72, 96), synth.synthetic_frame(72, 60, 80)]
    raw = hd.pack_candidates(det.detect_frames(frames))               # the host copy of the unsuppressed list
    counts = np.bincount(raw[:, 0], minlength=2)
    assert counts.min() > 20
    plan = hd.plan(72, 96)
    r, c = int(plan["feat_rows"][0]), int(plan["feat_cols"][0])
    before = hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r, c)
    # the four calls leave the resident result alone
    kept = hd.part_nms(2, 0.3, raw)
    gtb = np.zeros((2, 4))                                            # each frame's box: the centre hull of one of its records
    for f in range(2):
        pts = ev.centres(raw[raw[:, 0] == f][counts[f] // 2][None], 2)[0]
        gtb[f] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
    best, found = hd.best_overlap(gtb, 0.3, raw)
    hd.eval_pck(best, found, np.zeros((2, 2, 2)), [10.0, 10.0])
    hd.eval_apk(kept, [0, 1, 2], np.zeros((2, 2, 2)), [10.0, 10.0])
    assert same(hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r, c), before)
    assert same(kept, ev.part_nms(raw, 2, 2, 0.3)) and 0 < len(kept) < len(raw)
    wbest, wfound = ev.best_overlap(raw, 2, 2, gtb, 0.3)
    assert same(best, wbest) and same(found, wfound) and wfound.all()
    # the drivers: the same lists without the host copy
    assert same(hd.pack_candidates(det.testModel(frames, 0.3)), hd.pack_candidates(hd.unpack_candidates(kept.ravel(), len(kept))))
    got = det.testModelGtbox(frames, gtb, 0.3)
    assert all(g is not None for g in got)
    assert same(hd.pack_candidates(got), hd.pack_candidates(hd.unpack_candidates(wbest.ravel(), 2)))
    # the mirror methods on candidate objects
    cands = hd.unpack_candidates(raw.ravel(), len(raw))
    assert same(hd.pack_candidates(det.partNMS(cands, 0.3)), hd.pack_candidates(hd.unpack_candidates(kept.ravel(), len(kept))))
    poses = det.bestOverlap(cands, gtb, 0.3)
    gtp = ev.centres(wbest, 2) + 1.0
    pck, dist = det.evalPCK(poses, gtp, [2.0, 20.0])
    wpck, wdist = ev.eval_pck(hd.pack_candidates(poses), [1, 1], 2, gtp, [2.0, 20.0], 0.5)
    assert same(pck, wpck) and same(dist, wdist) and pck.tolist() == [0.5, 0.5]
    apk = det.evalAPK(hd.unpack_candidates(kept.ravel(), len(kept)), [0, 1, 2], gtp, [20.0, 20.0])
    wapk = ev.eval_apk(hd.pack_candidates(hd.unpack_candidates(kept.ravel(), len(kept))), 2, 2, [0, 1, 2], gtp, [20.0, 20.0], 0.5)
    assert all(same(a, b) for a, b in zip(apk, wapk))
    hd.close()
