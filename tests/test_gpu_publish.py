"""The candidate mask and the part-centre poses on the device (pbd_candidate_mask*, pbd_part_poses*), bit for bit against the numpy
yardsticks in partsbaseddetector_amd/publish.py: the person model's kept and unsuppressed lists of a 64 x 640x480 step, mixed frame
sizes, 1- and 4-channel frames, frames that are regions of a larger device image, device chains with no host copy of the list, bad
device lists, refusals, and the resident detect result left as it was."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, publish, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError
from partsbaseddetector_amd.pointcloud import PARTS_LITERAL, PinholeCamera, PointCloudClusterer as PCC

pytestmark = pytest.mark.gpu

CAM = PinholeCamera(525.0, 525.0, 319.5, 239.5)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def person():
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=64)
    yield hd
    hd.close()


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def fbits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def assert_poses(got, want):
    assert np.array_equal(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(fbits(g), fbits(w))


def device_payload(hd, rec, count=None, capacity=None):
    import torch
    cap = len(rec) if capacity is None else capacity
    pay = torch.zeros(1 + max(cap, 1) * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = len(rec) if count is None else count
    if len(rec):
        pay[1:1 + len(rec) * hd.stride] = torch.from_numpy(np.ascontiguousarray(rec, np.int32).ravel()).cuda()
    return pay, cap


def device_mask(hd, shapes, pay, cap, frames=None, frame_offset=0, in_place=False, region=False, fill=0):
    """(labels, masked, status) of pbd_candidate_mask_device; frames (host uint8) copied to the device, as regions of a larger
    image when `region`; outputs filled with `fill` first"""
    import torch
    labs = [torch.full((s[0] + 3, s[1] + 5), fill, dtype=torch.uint8, device="cuda") for s in shapes]   # pitch above the row
    ldesc = [(l.data_ptr(), l.stride(0)) for l in labs]
    cn, cdesc, mdesc, ins, outs = 0, None, None, None, None
    if frames is not None:
        cn = frames[0].shape[2]
        if region:
            bigs = [torch.full((f.shape[0] + 7, f.shape[1] + 9, cn), 77, dtype=torch.uint8, device="cuda") for f in frames]
            for b, f in zip(bigs, frames):
                b[3:3 + f.shape[0], 5:5 + f.shape[1]] = torch.from_numpy(f).cuda()
            ins = [b[3:3 + f.shape[0], 5:5 + f.shape[1]] for b, f in zip(bigs, frames)]
        else:
            ins = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
        outs = ins if in_place else [torch.full_like(i, fill) for i in ins]
        cdesc = [(i.data_ptr(), i.stride(0)) for i in ins]
        mdesc = [(o.data_ptr(), o.stride(0)) for o in outs]
    st = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.candidate_mask_device(shapes, pay.data_ptr(), cap, frame_offset, ldesc, cn, cdesc, mdesc, st.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    L = [l[:s[0], :s[1]].cpu().numpy() for l, s in zip(labs, shapes)]
    O = None if outs is None else [o.cpu().numpy() for o in outs]
    return L, O, int(st[0].item()), labs, outs


def check_list(hd, shapes, rec, frames, frame_offset=0):
    want = publish.frame_masks(shapes, rec, frame_offset)
    wm = [publish.masked_image(f, w) for f, w in zip(frames, want)]
    labs, masked = hd.candidate_mask(shapes, rec, frames, frame_offset)
    assert all(np.array_equal(g, w) for g, w in zip(labs, want))
    assert all(np.array_equal(g, w) for g, w in zip(masked, wm))
    inplace = [f.copy() for f in frames]
    labs2, masked2 = hd.candidate_mask(shapes, rec, inplace, frame_offset, labels=False, in_place=True)
    assert labs2 is None and all(np.array_equal(g, w) for g, w in zip(inplace, wm))
    pay, cap = device_payload(hd, rec)
    L, O, st, _, _ = device_mask(hd, shapes, pay, cap, frames, frame_offset)
    assert st == len(rec)
    assert all(np.array_equal(g, w) for g, w in zip(L, want))
    assert all(np.array_equal(g, w) for g, w in zip(O, wm))
    L, O, st, _, _ = device_mask(hd, shapes, pay, cap, frames, frame_offset, in_place=True, region=True)
    assert st == len(rec) and all(np.array_equal(g, w) for g, w in zip(L, want))
    assert all(np.array_equal(g, w) for g, w in zip(O, wm))
    return want


@pytest.fixture(scope="module")
def step(person):
    frames = [synth.synthetic_frame(100 + s, 480, 640, 3) for s in range(64)]
    person.set_nms(None)
    raw = raw_batch(person, frames)
    kept = person.suppress([(480, 640)] * 64, 0.1, raw)
    return frames, raw, kept


def test_kept_list_of_a_64_frame_step(person, step):
    frames, raw, kept = step
    assert 0 < len(kept) < len(raw)
    want = check_list(person, [(480, 640)] * 64, kept, frames)
    assert sum(int((w != 0).sum()) for w in want) > 0


def test_unsuppressed_list_of_a_64_frame_step(person, step):
    frames, raw, _ = step
    check_list(person, [(480, 640)] * 64, raw, frames)


def test_more_than_255_records_per_frame_mixed_sizes_and_channels(person):
    rng = np.random.default_rng(5)
    shapes = [(37, 300), (130, 70), (1, 1), (257, 129)]
    recs = []
    for f, (r, c) in enumerate(shapes):
        n = (0, 40, 3, 900)[f]
        rec = np.zeros((n, person.stride), np.int32)
        for i in range(n):
            k = int(rng.integers(1, person.max_parts + 1))
            rec[i, 0], rec[i, 6] = f + 3, k
            x0, y0 = int(rng.integers(-20, c + 5)), int(rng.integers(-20, r + 5))      # parts near one spot: small hulls
            for j in range(k):
                rec[i, 8 + 4 * j:12 + 4 * j] = (x0 + rng.integers(0, 6), y0 + rng.integers(0, 6), rng.integers(-2, max(c // 12, 2)),
                                                rng.integers(-2, max(r // 12, 2)))
        recs.append(rec)
    rec = np.concatenate(recs)
    for cn in (1, 3, 4):
        frames = [rng.integers(0, 256, (r, c, cn)).astype(np.uint8) for r, c in shapes]
        want = check_list(person, shapes, rec, frames, frame_offset=3)
    assert (want[3] == 255).any() and (want[3] == 1).any()


def test_device_chain_without_host_copies(person):
    import torch
    frames = np.stack([synth.synthetic_frame(60 + i, 480, 640, 3) for i in range(2)])
    depths = [synth.synthetic_depth(20 + f, 480, 640, np.float32) for f in range(2)]
    d_frames = torch.from_numpy(frames).cuda()
    d_depth = [torch.from_numpy(d).cuda() for d in depths]
    cap = 128
    pay = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    box = torch.zeros((cap, 6), dtype=torch.float64, device="cuda")
    cen = torch.zeros((cap, person.max_parts, 3), dtype=torch.float32, device="cuda")
    nc = torch.zeros(cap, dtype=torch.int32, device="cuda")
    dn = torch.zeros(cap, dtype=torch.int32, device="cuda")
    cnt = torch.full((cap,), -3, dtype=torch.int32, device="cuda")
    pos, ori, ev = (torch.zeros((cap, k), dtype=torch.float32, device="cuda") for k in (3, 4, 3))
    masked = d_frames.clone()
    labs = torch.zeros((2, 480, 640), dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    person.set_nms(0.1)
    try:
        person.check(person.lib.pbd_detect_batch_device_out(person.h, 2, d_frames.data_ptr(), 480, 640, 3, 5, pay.data_ptr(), cap))
    finally:
        person.set_nms(None)
    person.candidate_mask_device([(480, 640)] * 2, pay.data_ptr(), cap, 5, [(labs[f].data_ptr(), 640) for f in range(2)], 3,
                                 [(d_frames[f].data_ptr(), 1920) for f in range(2)], [(masked[f].data_ptr(), 1920) for f in range(2)],
                                 st.data_ptr())
    descs = [(d.data_ptr(), 480, 640, 640 * 4) for d in d_depth]
    person.boxes3d_camera_device(descs, 5, [(480, 640)] * 2, [CAM, CAM], PARTS_LITERAL, pay.data_ptr(), cap, 5, box.data_ptr(),
                                 cen.data_ptr(), nc.data_ptr(), dn.data_ptr())
    person.part_poses_device(pay.data_ptr(), cap, cen.data_ptr(), nc.data_ptr(), dn.data_ptr(), cnt.data_ptr(), pos.data_ptr(),
                             ori.data_ptr(), ev.data_ptr())
    torch.cuda.synchronize()
    p = pay.cpu().numpy()
    n = int(p[0])
    assert 0 < n <= cap and int(st[0].item()) == n
    rec = p[1:1 + n * person.stride].reshape(n, person.stride).copy()
    want = publish.frame_masks([(480, 640)] * 2, rec, 5)
    for f in range(2):
        assert np.array_equal(labs[f].cpu().numpy(), want[f])
        assert np.array_equal(masked[f].cpu().numpy(), publish.masked_image(frames[f], want[f]))
    got = (cnt.cpu().numpy()[:n], pos.cpu().numpy()[:n], ori.cpu().numpy()[:n], ev.cpu().numpy()[:n])
    c, k, d = cen.cpu().numpy()[:n], nc.cpu().numpy()[:n], dn.cpu().numpy()[:n]
    assert_poses(got, publish.part_poses(c, k, d))
    assert_poses(got, person.part_poses(c, k, d))                       # the host form equals the device form
    assert (cnt.cpu().numpy()[n:] == -3).all()                           # nothing written past the list
    cands = person.unpack_candidates(rec.ravel(), n)
    for cd in cands:
        cd.frame -= 5
    wb = PCC.computeBoundingBoxes(cands, [(480, 640)] * 2, depths, [CAM, CAM], PARTS_LITERAL, max_parts=person.max_parts)
    assert_poses(person.part_poses(wb[1], wb[2], wb[3]), publish.part_poses(wb[1], wb[2], wb[3]))
    assert (got[0] > 0).any()


def test_poses_of_hard_clouds(person):
    rng = np.random.default_rng(9)
    n, mp = 300, person.max_parts
    cen = (rng.standard_normal((n, mp, 3)) * np.array([0.3, 0.2, 0.05]) + np.array([0.0, 0.1, 2.0])).astype(np.float32)
    nc = rng.integers(0, mp + 1, n).astype(np.int32)
    dn = rng.integers(0, 2, n).astype(np.int32)
    for i in range(0, n, 7):
        cen[i, rng.integers(0, mp)] = (np.nan, 1, 1)
    for i in range(3, n, 11):
        cen[i, rng.integers(0, mp), rng.integers(0, 3)] = np.inf if i % 2 else -np.inf
    nc[:3] = (0, 1, 2)
    cen[20:30] = cen[20:30, :1]                                           # repeated points: a zero covariance
    cen[30:40, :, 2] = 2.0                                                # a flat cloud: ties in the eigenvalues
    got = person.part_poses(cen, nc, dn)
    want = publish.part_poses(cen, nc, dn)
    assert_poses(got, want)
    assert (got[0] == 0).any() and np.isnan(got[2]).any() and np.isfinite(got[2]).any()


def test_bad_device_lists_write_status_only(person, step):
    frames, raw, kept = step
    shapes = [(480, 640)] * 2
    rec = kept[kept[:, 0] < 2]
    fr = [frames[0], frames[1]]
    for count, cap, r in ((-1, len(rec), rec), (len(rec) + 1, len(rec), rec), (len(rec), len(rec), rec[::-1].copy())):
        pay, _ = device_payload(person, r, count=count, capacity=cap)
        L, O, st, _, _ = device_mask(person, shapes, pay, cap, fr, fill=123)
        assert st == -1
        assert all((l == 123).all() for l in L) and all((o == 123).all() for o in O)
    bad = rec.copy()
    bad[0, 0] = 7                                                          # a frame out of range
    pay, cap = device_payload(person, bad)
    assert device_mask(person, shapes, pay, cap, fr, fill=5)[2] == -1


def test_refusals_name_the_index_and_resident_result_untouched(person, step):
    import torch
    frames, raw, kept = step
    cap = person.max_candidates
    before = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, before.data_ptr(), cap))
    stage = person.get_stage(_lib.STAGE_ROOTV, 0, 0, *person.plan(480, 640)["feat_rows"][:1], person.plan(480, 640)["feat_cols"][0])
    rec = kept[kept[:, 0] < 2].copy()
    shapes = [(480, 640)] * 2
    ung = rec[::-1].copy()
    with pytest.raises(PbdError) as e:
        person.candidate_mask(shapes, ung, None)
    assert e.value.code == -1 and "record " in str(e.value)
    oor = rec.copy()
    oor[-1, 0] = 2
    with pytest.raises(PbdError) as e:
        person.candidate_mask(shapes, oor, None)
    assert e.value.code == -1 and f"record {len(rec) - 1}" in str(e.value)
    np_bad = rec.copy()
    np_bad[1, 6] = person.max_parts + 1
    with pytest.raises(PbdError) as e:
        person.candidate_mask(shapes, np_bad, None)
    assert "record 1" in str(e.value)
    with pytest.raises(PbdError) as e:
        person.candidate_mask([(480, 640), (0, 640)], rec, None)
    assert "frame 1" in str(e.value)
    with pytest.raises(PbdError) as e:
        person.candidate_mask([(480, 640), (70000, 640)], rec, None)
    assert "frame 1" in str(e.value)
    with pytest.raises(PbdError) as e:
        person.candidate_mask(shapes, rec, [np.zeros((480, 640, 2), np.uint8)] * 2)
    assert e.value.code == -1
    labs = np.zeros((2, 480, 640), np.uint8)
    ir = np.array([480, 480], np.int32)
    ic = np.array([640, 640], np.int32)
    lp = (C.c_void_p * 2)(labs[0].ctypes.data, labs[1].ctypes.data)
    ls = (C.c_size_t * 2)(640, 639)                                        # a pitch below the row
    rc = person.lib.pbd_candidate_mask(person.h, 2, _lib.ptr(ir, C.c_int), _lib.ptr(ic, C.c_int), rec.ctypes.data, len(rec), 0, lp, ls, 0,
                                       None, None, None, None)
    assert rc == -1 and b"frame 1" in person.lib.pbd_last_error(person.h)
    cen = np.zeros((2, person.max_parts, 3), np.float32)
    with pytest.raises(PbdError) as e:
        person.part_poses(cen, np.array([1, person.max_parts + 1], np.int32), np.ones(2, np.int32))
    assert "record 1" in str(e.value)
    after = torch.zeros_like(before)
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, after.data_ptr(), cap))
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    stage2 = person.get_stage(_lib.STAGE_ROOTV, 0, 0, *person.plan(480, 640)["feat_rows"][:1], person.plan(480, 640)["feat_cols"][0])
    assert np.array_equal(np.asarray(stage).view(np.uint8), np.asarray(stage2).view(np.uint8))


def test_detector_mask_and_part_poses(person):
    model = M.synthetic_person_model()
    det = detector.PartsBasedDetector(device=0)
    det.distributeModel(model)
    im = synth.synthetic_frame(3, 480, 640, 3)
    depth = synth.synthetic_depth(3, 480, 640, np.float32)
    cands = det.detect(im)
    cands = det.suppress(cands, (480, 640), 0.1)
    labels, masked = det.mask(cands, (480, 640), im.copy())
    want = detector.Candidate.mask((480, 640), cands)
    assert np.array_equal(labels[0], want) and np.array_equal(masked[0], publish.masked_image(im, want))
    boxes, cen, nc, dn = det.computeBoundingBoxes(cands, depth, (480, 640), CAM)
    assert_poses(det.partPoses(cen, nc, dn), publish.part_poses(cen, nc, dn))
