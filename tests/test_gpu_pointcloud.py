"""Camera boxes, part centres and object clusters on the device (pbd_boxes3d_camera*, pbd_cluster_objects*;
PartsBasedDetector.computeBoundingBoxes / .clusterObjects).

The yardsticks are partsbaseddetector_amd/pointcloud.py (pinned on the CPU by tests/test_pointcloud_cpu.py).  Comparisons are of
BIT PATTERNS: float64 for the boxes, float32 for the centres, exact index lists.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError
from partsbaseddetector_amd.pointcloud import PARTS_LITERAL, PARTS_XY, PinholeCamera, PointCloudClusterer as PCC, cloud_from_depth

pytestmark = pytest.mark.gpu
CAM = PinholeCamera(525.0, 525.0, 319.5, 239.5)
CAM2 = PinholeCamera(610.5, 600.25, 410.0, 300.5, 0.125, -0.75)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def person():
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=2)
    yield hd
    hd.close()


def bits(a, dt):
    return np.ascontiguousarray(np.asarray(a, dt)).view(np.uint64 if dt == np.float64 else np.uint32)


def assert_same(got, want, dt):
    g, w = bits(got, dt), bits(want, dt)
    bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0] if g.size else []
    assert g.shape == w.shape and not len(bad), (len(bad), np.asarray(got)[bad[:2]], np.asarray(want)[bad[:2]])


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def record(hd, frame, parts):
    r = np.zeros(hd.stride, np.int32)
    parts = np.asarray(parts, np.int32).reshape(-1, 4)
    r[0], r[6] = frame, len(parts)
    r[8:8 + parts.size] = parts.ravel()
    return r


def mirror_camera(hd, rec, depths, shapes, cams, mode=PARTS_LITERAL, frame_offset=0):
    cands = hd.unpack_candidates(np.ascontiguousarray(rec).ravel(), len(rec))
    for c in cands:
        c.frame -= frame_offset
    return PCC.computeBoundingBoxes(cands, shapes, depths, cams, mode, max_parts=hd.max_parts)


def check_camera(hd, rec, depths, shapes, cams, mode=PARTS_LITERAL):
    got = hd.boxes3d_camera(depths, shapes, cams, rec, mode)
    want = mirror_camera(hd, rec, depths, shapes, cams, mode)
    assert_same(got[0], want[0], np.float64)
    assert_same(got[1], want[1], np.float32)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    return got


def check_clusters(hd, clouds, boxes, frames):
    cen, cnt, idx = hd.cluster_objects(clouds, boxes, frames)
    wc, wi = PCC.clusterObjects(clouds, boxes, frames)
    assert_same(cen, wc, np.float32)
    assert list(cnt) == [len(v) for v in wi]
    assert np.array_equal(idx, np.concatenate(wi + [np.zeros(0, np.int64)]))
    return cen, cnt, wi


# ---- the person model on synthetic depth ---------------------------------------------------------------------------------------
def test_person_detections_boxes_centres_and_clusters(person):
    frames = [synth.synthetic_frame(40 + i, 480, 640, 3) for i in range(2)]
    person.set_nms(0.1)
    rec = raw_batch(person, frames)
    person.set_nms(None)
    assert len(rec) > 0
    depths = [synth.synthetic_depth(7 + f, 480, 640, np.float32) for f in range(2)]
    shapes, cams = [(480, 640)] * 2, [CAM, CAM2]
    for mode in (PARTS_LITERAL, PARTS_XY):
        box, cen, nc, dn = check_camera(person, rec, depths, shapes, cams, mode)
    clouds = [cloud_from_depth(depths[f], cams[f]) for f in range(2)]
    cen, cnt, _ = check_clusters(person, clouds, box, rec[:, 0])
    assert (cnt > 0).any()
    # PartsBasedDetector forms
    det = detector.PartsBasedDetector()
    det.distributeModel(M.synthetic_person_model())
    cands = person.unpack_candidates(rec.ravel(), len(rec))
    got = det.computeBoundingBoxes(cands, depths, shapes, cams)
    assert_same(got[0], box, np.float64)
    c2, lists = det.clusterObjects(clouds, got[0], [c.frame for c in cands])
    assert_same(c2, cen, np.float32)
    assert [len(v) for v in lists] == list(cnt)
    det.hd.close()


def test_frames_of_different_sizes_and_cameras_nan_cubes_and_parts_leaving_the_depth(person):
    depths = [synth.synthetic_depth(3, 240, 320, np.float32), synth.synthetic_depth(4, 300, 500, np.float32),
              np.zeros((200, 200), np.float32)]
    shapes = [(240, 320), (150, 250), (200, 200)]       # frame 1: depth twice the colour size
    cams = [CAM, CAM2, CAM]
    rng = np.random.default_rng(1)
    recs = []
    for i in range(24):
        f = i % 3
        rows, cols = shapes[f]
        parts = [(int(rng.integers(-20, cols)), int(rng.integers(-20, rows)), int(rng.integers(1, 60)), int(rng.integers(1, 60)))
                 for _ in range(int(rng.integers(1, 26)))]
        recs.append(record(person, f, parts))
    rec = np.stack(recs)
    for mode in (PARTS_LITERAL, PARTS_XY):
        box, cen, nc, dn = check_camera(person, rec, depths, shapes, cams, mode)
        assert (nc[2::3] == 0).all() and (box[2::3] == 0).all()      # the all-zero depth: NaN cubes, skipped records
        assert (dn == 0).any()
    clouds = [cloud_from_depth(depths[f], cams[f]) for f in range(3)]
    check_clusters(person, clouds, box, rec[:, 0])


def test_device_chain_without_host_copies(person):
    import torch
    frames = np.stack([synth.synthetic_frame(60 + i, 480, 640, 3) for i in range(2)])
    depths = [synth.synthetic_depth(20 + f, 480, 640, np.float32) for f in range(2)]
    clouds = [cloud_from_depth(depths[f], [CAM, CAM2][f]) for f in range(2)]
    d_frames = torch.from_numpy(frames).cuda()
    d_depth = [torch.from_numpy(d).cuda() for d in depths]
    big = torch.full((2, 500, 700, 4), float("nan"), dtype=torch.float32, device="cuda")    # clouds as regions of a larger buffer
    for f in range(2):
        big[f, 10:490, 30:670, :3] = torch.from_numpy(clouds[f]).cuda()
    cap = 128
    pay = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    box = torch.zeros((cap, 6), dtype=torch.float64, device="cuda")
    cen = torch.zeros((cap, person.max_parts, 3), dtype=torch.float32, device="cuda")
    nc = torch.zeros(cap, dtype=torch.int32, device="cuda")
    dn = torch.zeros(cap, dtype=torch.int32, device="cuda")
    oc = torch.zeros((cap, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(cap, dtype=torch.int32, device="cuda")
    idx = torch.full((1 << 21,), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    person.set_nms(0.1)
    person.check(person.lib.pbd_detect_batch_device_out(person.h, 2, d_frames.data_ptr(), 480, 640, 3, 5, pay.data_ptr(), cap))
    descs = [(d.data_ptr(), 480, 640, 640 * 4) for d in d_depth]
    person.boxes3d_camera_device(descs, 5, [(480, 640)] * 2, [CAM, CAM2], PARTS_LITERAL, pay.data_ptr(), cap, 5, box.data_ptr(),
                                 cen.data_ptr(), nc.data_ptr(), dn.data_ptr())
    cdesc = [(big[f, 10, 30].data_ptr(), 480, 640, 16, 700 * 16) for f in range(2)]
    person.cluster_objects_device(cdesc, pay.data_ptr(), cap, 5, box.data_ptr(), 1 << 22, idx.numel(), oc.data_ptr(),
                                  cnt.data_ptr(), idx.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    person.set_nms(None)
    p = pay.cpu().numpy()
    n = int(p[0])
    assert 0 < n <= cap
    rec = p[1:1 + n * person.stride].reshape(n, person.stride).copy()
    want = mirror_camera(person, rec, depths, [(480, 640)] * 2, [CAM, CAM2], frame_offset=5)
    assert_same(box.cpu().numpy()[:n], want[0], np.float64)
    assert np.array_equal(nc.cpu().numpy()[:n], want[2]) and np.array_equal(dn.cpu().numpy()[:n], want[3])
    c = cen.cpu().numpy()[:n]
    for i in range(n):
        assert_same(c[i, :want[2][i]], want[1][i, :want[2][i]], np.float32)
    wc, wi = PCC.clusterObjects(clouds, want[0], rec[:, 0] - 5)
    s = st.cpu().numpy()
    assert s[1] == sum(len(v) for v in wi) and s[0] >= s[1]
    assert_same(oc.cpu().numpy()[:n], wc, np.float32)
    assert list(cnt.cpu().numpy()[:n]) == [len(v) for v in wi]
    ix = idx.cpu().numpy()
    assert np.array_equal(ix[:s[1]], np.concatenate(wi + [np.zeros(0, np.int64)])) and (ix[s[1]:] == -7).all()


def device_inputs(hd, clouds, boxes, frames):
    import torch
    d_clouds = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]
    n = len(boxes)
    rec = np.zeros((n, hd.stride), np.int32)
    rec[:, 0] = frames
    pay = torch.from_numpy(np.concatenate([[n], rec.ravel()]).astype(np.int32)).cuda()
    bx = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).cuda()
    descs = [(d.data_ptr(),) + hd.cloud_desc(c)[1:] for d, c in zip(d_clouds, clouds)]
    return d_clouds, pay, bx, descs


def test_capacity_overflow_both_forms_and_minus_one_payload(person):
    import torch
    depth = synth.synthetic_depth(9, 120, 160, np.float32)
    cloud = cloud_from_depth(depth, CAM)
    P = cloud.reshape(-1, 3)
    good = P[np.isfinite(P).all(axis=1)]
    lo, hi = good.min(axis=0), good.max(axis=0)
    boxes = np.array([[lo[0], lo[1], lo[2], hi[1] - lo[1], hi[0] - lo[0], hi[2] - lo[2]]] * 3)
    cen, cnt, idx = person.cluster_objects([cloud], boxes, [0, 0, 0])
    total = int(cnt.sum())
    assert total > 100
    with pytest.raises(PbdError) as e:
        person.cluster_objects([cloud], boxes, [0, 0, 0], index_capacity=total - 1)
    assert e.value.code == -4 and e.value.needed == total
    # the device form: a crop workspace too small, then an index capacity too small; guards after every output
    d_clouds, pay, bx, descs = device_inputs(person, [cloud], boxes, [0, 0, 0])
    cropped = None
    guard = 12345
    for crop_cap, index_cap in ((50, 10 ** 6), (10 ** 6, total - 1), (10 ** 6, total)):
        oc = torch.full((4, 3), 9.0, dtype=torch.float32, device="cuda")
        cn = torch.full((4,), guard, dtype=torch.int32, device="cuda")
        ix = torch.full((index_cap + 64,), guard, dtype=torch.int32, device="cuda")
        st = torch.zeros(3, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        person.cluster_objects_device(descs, pay.data_ptr(), 3, 0, bx.data_ptr(), crop_cap, index_cap, oc.data_ptr(), cn.data_ptr(),
                                      ix.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
        s, o, c, i = st.cpu().numpy(), oc.cpu().numpy(), cn.cpu().numpy(), ix.cpu().numpy()
        assert o[3, 0] == 9.0 and c[3] == guard and s[2] == 0 and (i[index_cap:] == guard).all()
        if crop_cap == 50:
            assert s[0] > 50 and s[1] == -1 and (c[:3] == 0).all() and np.isnan(o[:3]).all() and (i == guard).all()
            cropped = s[0]
        elif index_cap < total:
            assert s[0] == cropped and s[1] == total and (i == guard).all()
            assert_same(o[:3], cen, np.float32) and list(c[:3]) == list(cnt)
        else:
            assert s[1] == total and np.array_equal(i[:total], idx)
    # a -1 payload (a suppression overflow) writes no box
    pay[0] = -1
    oc = torch.full((3, 3), 9.0, dtype=torch.float32, device="cuda")
    st = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    person.cluster_objects_device(descs, pay.data_ptr(), 3, 0, bx.data_ptr(), 10 ** 6, 10 ** 6, oc.data_ptr(), cn.data_ptr(),
                                  ix.data_ptr(), st.data_ptr())
    box = torch.full((3, 6), 4.0, dtype=torch.float64, device="cuda")
    dd = torch.from_numpy(depth).cuda()
    cen3 = torch.zeros((3, person.max_parts, 3), dtype=torch.float32, device="cuda")
    cen3.fill_(6.0)
    nc = torch.full((3,), 8, dtype=torch.int32, device="cuda")
    dn = torch.full((3,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    person.boxes3d_camera_device([(dd.data_ptr(), 120, 160, 640)], 5, [(120, 160)], [CAM], 0, pay.data_ptr(), 3, 0, box.data_ptr(),
                                 cen3.data_ptr(), nc.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    assert (oc.cpu().numpy() == 9.0).all() and (st.cpu().numpy() == [0, 0]).all()
    assert (box.cpu().numpy() == 4.0).all() and (cen3.cpu().numpy() == 6.0).all()
    assert (nc.cpu().numpy() == 8).all() and (dn.cpu().numpy() == 9).all()


def test_refusals_and_resident_result_untouched(person):
    import torch
    frames = [synth.synthetic_frame(5, 480, 640, 3)]
    rec = raw_batch(person, frames)
    cap = person.max_candidates
    before = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, before.data_ptr(), cap))
    depth = synth.synthetic_depth(1, 480, 640, np.float32)
    with pytest.raises(PbdError) as e:
        person.boxes3d_camera([synth.synthetic_depth(1, 480, 640, np.uint16)], [(480, 640)], [CAM], rec)
    assert e.value.code == -2
    for bad in (PinholeCamera(0.0, 525, 1, 1), PinholeCamera(525, float("nan"), 1, 1), PinholeCamera(float("inf"), 525, 1, 1)):
        with pytest.raises(PbdError) as e:
            person.boxes3d_camera([depth], [(480, 640)], [bad], rec)
        assert e.value.code == -1 and "frame 0" in str(e.value)
    with pytest.raises(PbdError) as e:
        person.boxes3d_camera([depth], [(480, 640)], [CAM], rec, parts_mode=2)
    assert e.value.code == -1
    cloud = cloud_from_depth(depth, CAM)
    descs = _lib.cloud_array([(cloud.ctypes.data, 480, 640, 8, 640 * 12)])             # a point stride below 12
    need = C.c_int()
    out = np.zeros(8, np.float32)
    i32 = np.zeros(8, np.int32)
    bx = np.zeros((1, 6))
    fr = np.zeros(1, np.int32)
    assert person.lib.pbd_cluster_objects(person.h, 1, descs, bx.ctypes.data, fr.ctypes.data, 1, out.ctypes.data, i32.ctypes.data,
                                          i32.ctypes.data, 8, C.byref(need)) == -1
    descs = _lib.cloud_array([(cloud.ctypes.data, 480, 640, 12, 640 * 12 - 4)])        # a row stride below the row
    assert person.lib.pbd_cluster_objects(person.h, 1, descs, bx.ctypes.data, fr.ctypes.data, 1, out.ctypes.data, i32.ctypes.data,
                                          i32.ctypes.data, 8, C.byref(need)) == -1
    fr[0] = 1                                                                           # a frame outside the clouds
    descs = _lib.cloud_array([(cloud.ctypes.data, 480, 640, 12, 640 * 12)])
    assert person.lib.pbd_cluster_objects(person.h, 1, descs, bx.ctypes.data, fr.ctypes.data, 1, out.ctypes.data, i32.ctypes.data,
                                          i32.ctypes.data, 8, C.byref(need)) == -1
    assert b"box 0" in person.lib.pbd_last_error(person.h)
    d = torch.from_numpy(cloud).cuda()
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(PbdError):                                                       # a device stride not a multiple of 4
        person.cluster_objects_device([(d.data_ptr(), 480, 640, 14, 640 * 14)], before.data_ptr(), 1, 0, d.data_ptr(), 10, 10,
                                      d.data_ptr(), d.data_ptr(), d.data_ptr(), st.data_ptr())
    after = torch.zeros_like(before)
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, after.data_ptr(), cap))
    torch.cuda.synchronize()
    assert torch.equal(before, after)


def test_full_frame_boxes_crop_over_50000_points(person):
    depth = synth.synthetic_depth(31, 480, 640, np.float32)
    cloud = cloud_from_depth(depth, CAM)
    recs = np.stack([record(person, 0, [(40, 30, 500, 400)]), record(person, 0, [(200, 100, 300, 300), (250, 150, 50, 60)]),
                     record(person, 0, [(0, 0, 640, 480)])])
    box, _, _, _ = check_camera(person, recs, [depth], [(480, 640)], [CAM])
    cen, cnt, wi = check_clusters(person, [cloud], box, recs[:, 0])
    assert max(len(PCC.crop(cloud, b)) for b in box) > 50000


def test_randomised_small_scenes(person):
    """200 seeded scenes: clumps of points a few mm apart, duplicates, points at the radius, non-finite points; organized and
    unorganized clouds, several clouds and boxes per call"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pc_cpu", os.path.join(os.path.dirname(__file__), "test_pointcloud_cpu.py"))
    cpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cpu)
    for batch in range(20):
        clouds, boxes, frames = [], [], []
        for k in range(10):
            rng = np.random.default_rng(1000 * batch + k)
            pts = cpu.scene(rng, 60)
            if k % 2 == 0 and len(pts) % 4 == 0:
                pts = pts.reshape(4, -1, 3)
            clouds.append(pts)
            for _ in range(2):
                boxes.append(cpu.box_around(pts.reshape(-1, 3), rng))
                frames.append(k)
        check_clusters(person, clouds, np.array(boxes), np.array(frames))
