"""3-D boxes from a depth image on the device (pbd_boxes3d, pbd_boxes3d_device; Handle.boxes3d,
PartsBasedDetector.boundingBoxes3D).

The yardstick is Candidate.boundingBox3D, the numpy mirror of include/Candidate.hpp:140-216.  Every comparison is of the
float64 BIT PATTERNS of the six values per record, NaN boxes included.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import Candidate, PbdError

pytestmark = pytest.mark.gpu
NAN_BOX = np.array([np.nan, np.nan, np.nan, 0, 0, 0])


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def person():
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=2)
    yield hd
    hd.close()


def candidates(hd, rec):
    return hd.unpack_candidates(np.ascontiguousarray(rec).ravel(), len(rec))


def mirror(hd, rec, depths, shapes, frame_offset=0):
    out = np.zeros((len(rec), 6))
    for i, c in enumerate(candidates(hd, rec)):
        f = c.frame - frame_offset
        out[i] = c.boundingBox3D(shapes[f], depths[f])
    return out


def assert_bits(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert got.shape == want.shape and not len(bad), (len(bad), got[bad[:3]] if len(bad) else None, want[bad[:3]] if len(bad) else None)


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


# ---- 1. the person model on synthetic frames ------------------------------------------------------------------------------------
def test_person_nms_off_and_on_every_code_both_sizes(person):
    frames = [synth.synthetic_frame(40 + i, 480, 640, 3) for i in range(2)]
    person.set_nms(None)
    raw = raw_batch(person, frames)
    person.set_nms(0.1)
    kept = raw_batch(person, frames)
    person.set_nms(None)
    assert len(raw) >= 100 and 0 < len(kept) < len(raw), (len(raw), len(kept))
    shapes = [(480, 640)] * 2
    for dt in (np.uint16, np.float32, np.float64):
        full = [synth.synthetic_depth(7 + f, 480, 640, dt) for f in range(2)]
        half = [synth.synthetic_depth(9 + f, 240, 320, dt) for f in range(2)]
        for rec, depths in ((raw, full), (kept, full), (kept, half)):
            got = person.boxes3d(depths, shapes, rec)
            assert_bits(got, mirror(person, rec, depths, shapes))
    # the list's own z values are real depths: most boxes are not the NaN box
    assert np.isfinite(got[:, 2]).mean() > 0.5


def test_boundingBoxes3D_from_candidates(person):
    det = detector.PartsBasedDetector(device=0, nms=0.1)
    det.distributeModel(M.synthetic_person_model())
    im = synth.synthetic_frame(61, 480, 640, 3)
    depth = synth.synthetic_depth(61, 480, 640, np.uint16)
    cands = det.detect(im, depth)
    assert np.array_equal(det.hd.pack_candidates(cands), det.hd.pack_candidates(det.detect(im)))   # depth is still ignored
    assert len(cands) > 0
    got = det.boundingBoxes3D(cands, depth, (480, 640))
    assert got.dtype == np.float64 and got.shape == (len(cands), 6)
    assert_bits(got, np.array([c.boundingBox3D((480, 640), depth) for c in cands]).reshape(-1, 6))
    det.hd.close()


# ---- 2. hand-built records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 399, 400, 401, 12345])
def test_sample_count_edges(person, m):
    """one part (boundingBoxNorm of one centroid is empty): M = the part's area of a hole-free depth image"""
    w, h = {1: (1, 1), 2: (2, 1), 399: (21, 19), 400: (20, 20), 401: (401, 1), 12345: (823, 15)}[m]
    rng = np.random.default_rng(m)
    depth = rng.integers(-4, 40, size=(1000, 1000)).astype(np.float32) / 4
    depth[depth == 0] = 0.5
    rec = np.stack([record(person, 0, [[3, 5, w, h]]), record(person, 0, [[990 - w, 980 - h, w, h]] * 3)])
    got = person.boxes3d([depth], [(1000, 1000)], rec)
    assert_bits(got, mirror(person, rec, [depth], [(1000, 1000)]))


def test_inf_negative_and_nan_boxes(person):
    rng = np.random.default_rng(5)
    depth = (rng.standard_normal((480, 640)) * 3).astype(np.float32)
    depth[rng.random((480, 640)) < 0.05] = np.inf
    depth[rng.random((480, 640)) < 0.05] = -np.inf
    depth[rng.random((480, 640)) < 0.05] = np.nan
    depth[rng.random((480, 640)) < 0.05] = 0
    depth[100:140, 200:260] = 0                           # a hole
    depth[300:320, 10:30] = -2.5                          # negative plateau
    parts = [[10 + 23 * k, 20 + 15 * k, 30, 25] for k in range(26)]
    recs = [record(person, 0, parts),
            record(person, 0, [[200, 100, 60, 40], [0, 0, 300, 300]]),          # first box all holes: NaN box
            record(person, 0, [[-50, -50, 20, 20], [700, 10, 5, 5], [10, 300, 20, 20]]),   # leading boxes outside the frame
            record(person, 0, [[10, 300, 20, 20]] * 5),
            record(person, 0, [[630, 470, 40, 40], [0, 0, 1, 1]])]
    rec = np.stack(recs)
    got = person.boxes3d([depth], [(480, 640)], rec)
    want = mirror(person, rec, [depth], [(480, 640)])
    assert_bits(got, want)
    assert_bits(got[1:2], NAN_BOX[None])


def test_all_boxes_empty_and_empty_after_scaling(person):
    tiny = np.full((2, 3), 1.5, np.float32)               # 2 x 3 depth under a VGA frame: every scaled box is empty
    rec = np.stack([record(person, 0, [[10, 10, 100, 100], [50, 60, 30, 30]]), record(person, 0, [[0, 0, 640, 480]])])
    got = person.boxes3d([tiny], [(480, 640)], rec)
    assert_bits(got[:1], NAN_BOX[None])
    assert_bits(got, mirror(person, rec, [tiny], [(480, 640)]))
    # a box of width 1 vanishes at half resolution; the next one has samples
    half = synth.synthetic_depth(3, 240, 320, np.uint16, holes=False)
    rec = np.stack([record(person, 0, [[101, 100, 1, 40], [200, 200, 30, 30]])])
    assert_bits(person.boxes3d([half], [(480, 640)], rec), mirror(person, rec, [half], [(480, 640)]))


def test_non_integer_ratio_and_16u_equals_32f(person):
    d16 = synth.synthetic_depth(21, 370, 500, np.uint16)
    parts = [[5 + 24 * k, 7 + 17 * k, 40, 33] for k in range(26)]
    rec = np.stack([record(person, 0, parts), record(person, 0, parts[3:9])])
    got16 = person.boxes3d([d16], [(480, 640)], rec)
    assert_bits(got16, mirror(person, rec, [d16], [(480, 640)]))
    assert_bits(person.boxes3d([d16.astype(np.float32)], [(480, 640)], rec), got16)
    d64 = d16.astype(np.float64) / 1000
    d64[::7, ::5] = 1e-50                                 # rounds to 0.0f: not a sample
    assert_bits(person.boxes3d([d64], [(480, 640)], rec), mirror(person, rec, [d64], [(480, 640)]))


def test_record_covering_most_of_1080p(person):
    """about 10 M samples in one record, next to small ones"""
    depth = synth.synthetic_depth(77, 1080, 1920, np.float32)
    big = [[10, 12, 1900, 1060], [0, 0, 1920, 1080], [30, 5, 1850, 1070], [960, 540, 900, 500]]
    rec = np.stack([record(person, 0, [[100, 100, 40, 40]]), record(person, 0, big), record(person, 0, [[1500, 900, 64, 64]] * 2)])
    got = person.boxes3d([depth], [(1080, 1920)], rec)
    assert_bits(got, mirror(person, rec, [depth], [(1080, 1920)]))


# ---- 3. the device form ------------------------------------------------------------------------------------------------------------
def test_device_form_after_device_out_with_offset(person):
    import torch
    frames = np.stack([synth.synthetic_frame(80 + i, 480, 640, 3) for i in range(2)])
    d_frames = torch.from_numpy(frames).cuda()
    depths = [synth.synthetic_depth(80 + i, 480, 640, np.float32, inf=True) for i in range(2)]
    d_depth = [torch.from_numpy(d).cuda() for d in depths]
    torch.cuda.synchronize()
    person.set_nms(0.1)
    cap = 512
    pay = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    person.check(person.lib.pbd_detect_batch_device_out(person.h, 2, d_frames.data_ptr(), 480, 640, 3, 5, pay.data_ptr(), cap))
    out = torch.full((cap, 6), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    descs = [(d.data_ptr(), 480, 640, d.stride(0) * 4) for d in d_depth]
    person.boxes3d_device(descs, 5, [(480, 640)] * 2, pay.data_ptr(), cap, 5, out.data_ptr())
    person.check(person.lib.pbd_synchronize(person.h))
    person.set_nms(None)
    p = pay.cpu().numpy()
    n = int(p[0])
    assert 0 < n <= cap
    rec = p[1:1 + n * person.stride].reshape(n, person.stride)
    assert set(np.unique(rec[:, 0])) <= {5, 6}
    got = out.cpu().numpy()
    want = person.boxes3d(depths, [(480, 640)] * 2, rec, frame_offset=5)
    assert_bits(got[:n], want)
    assert_bits(want, mirror(person, rec, depths, [(480, 640)] * 2, frame_offset=5))
    assert (got[n:] == 7.0).all()
    # a record of another frame range gets six NaNs (not the NaN box)
    out.fill_(7.0)
    torch.cuda.synchronize()
    person.boxes3d_device(descs[:1], 5, [(480, 640)], pay.data_ptr(), cap, 5, out.data_ptr())
    person.check(person.lib.pbd_synchronize(person.h))
    g = out.cpu().numpy()[:n]
    assert np.isnan(g[rec[:, 0] == 6]).all() and np.array_equal(g[rec[:, 0] == 5].view(np.uint64), want[rec[:, 0] == 5].view(np.uint64))
    # a -1 payload (suppression overflow) writes nothing
    pay[0] = -1
    out.fill_(7.0)
    torch.cuda.synchronize()
    person.boxes3d_device(descs, 5, [(480, 640)] * 2, pay.data_ptr(), cap, 5, out.data_ptr())
    person.check(person.lib.pbd_synchronize(person.h))
    assert (out.cpu().numpy() == 7.0).all()


def test_mixed_sizes_and_a_device_region():
    import torch
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=3)
    sizes = [(480, 640), (360, 500), (300, 420)]
    frames = [synth.synthetic_frame(90 + i, r, c, 3) for i, (r, c) in enumerate(sizes)]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in frames])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, 3, descs, 3, 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    rec = buf[: n.value * hd.stride].reshape(n.value, hd.stride)
    assert len(np.unique(rec[:, 0])) >= 2
    depths = [synth.synthetic_depth(90 + i, r // (1 + i % 2), c // (1 + i % 2), np.uint16) for i, (r, c) in enumerate(sizes)]
    got = hd.boxes3d(depths, sizes, rec)
    assert_bits(got, mirror(hd, rec, depths, sizes))
    # the depth of a frame other than 0 as a region of a larger device image, read in place
    fs = int(rec[-1, 0])
    assert fs > 0
    big = synth.synthetic_depth(5, 700, 900, np.uint16)
    y0, x0 = 123, 211
    crop = big[y0:y0 + depths[fs].shape[0], x0:x0 + depths[fs].shape[1]]
    d_big = torch.from_numpy(big.view(np.int16)).cuda()    # the uint16 bits
    pitch = 900 * 2
    sel = rec[rec[:, 0] == fs]
    pay = torch.from_numpy(np.concatenate([[len(sel)], sel.ravel()]).astype(np.int32)).cuda()
    out = torch.zeros((len(sel), 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hd.boxes3d_device([(d_big.data_ptr() + y0 * pitch + x0 * 2, crop.shape[0], crop.shape[1], pitch)], 2, [sizes[fs]],
                      pay.data_ptr(), len(sel), fs, out.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    want = hd.boxes3d([np.ascontiguousarray(crop)], [sizes[fs]], sel, frame_offset=fs)
    assert_bits(out.cpu().numpy(), want)
    assert_bits(want, mirror(hd, sel, [crop], [sizes[fs]], frame_offset=fs))
    hd.close()


def test_double_handle_same_boxes(person):
    frames = [synth.synthetic_frame(50, 480, 640, 3)]
    rec = raw_batch(person, frames)
    hd64 = detector.Handle(M.synthetic_person_model(), device=0, max_batch=1, real_type=_lib.REAL_F64)
    assert hd64.stride == person.stride
    depth = synth.synthetic_depth(50, 480, 640, np.float64)
    assert_bits(hd64.boxes3d([depth], [(480, 640)], rec), person.boxes3d([depth], [(480, 640)], rec))
    hd64.close()


# ---- 4. refusals and the resident result ----------------------------------------------------------------------------------------
def test_refusals_and_resident_result_untouched(person):
    import torch
    frames = [synth.synthetic_frame(60 + i, 480, 640, 3) for i in range(2)]
    rec = raw_batch(person, frames)
    d_frames = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    cap = len(rec) + 8
    before = torch.zeros(1 + cap * person.stride, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, before.data_ptr(), cap))
    plan = person.plan(480, 640)
    stage = person.get_stage(_lib.STAGE_ROOTV, 1, 3, int(plan["feat_rows"][3]), int(plan["feat_cols"][3]))
    depth = synth.synthetic_depth(60, 480, 640, np.uint16)
    good = person.boxes3d([depth] * 2, [(480, 640)] * 2, rec)

    def call(depth_code=2, rows=480, cols=640, pitch=1280, shape=(480, 640), recs=rec, nframes=2):
        descs = _lib.frame_array([(depth.ctypes.data, rows, cols, pitch)] * nframes)
        ir = np.array([shape[0]] * nframes, np.int32)
        ic = np.array([shape[1]] * nframes, np.int32)
        out = np.zeros((max(len(recs), 1), 6))
        r = np.ascontiguousarray(recs, np.int32)
        return person.lib.pbd_boxes3d(person.h, nframes, descs, depth_code, _lib.ptr(ir, C.c_int), _lib.ptr(ic, C.c_int),
                                      r.ctypes.data, len(r), 0, out.ctypes.data)

    assert call() == 0
    assert call(depth_code=3) == -1 and b"depth code 3" in person.lib.pbd_last_error(person.h)
    assert call(rows=0) == -1 and b"frame 0" in person.lib.pbd_last_error(person.h)
    assert call(shape=(480, -1)) == -1
    assert call(pitch=1278) == -1 and b"stride" in person.lib.pbd_last_error(person.h)
    assert call(nframes=1) == -1 and b"record" in person.lib.pbd_last_error(person.h)   # frame 1 out of range
    person.check(person.lib.pbd_detect_batch_submit(person.h, 2, _lib.ptr_array(frames), 480, 640, 3, 640 * 3))
    assert call() == -5
    buf = np.zeros(person.max_candidates * person.stride, np.int32)
    n = C.c_int()
    person.check(person.lib.pbd_detect_batch_wait(person.h, buf.ctypes.data, person.max_candidates, C.byref(n)))
    # the batch just waited for is the resident result again; a boxes3d call leaves it readable
    assert_bits(person.boxes3d([depth] * 2, [(480, 640)] * 2, rec), good)
    after = torch.zeros_like(before)
    torch.cuda.synchronize()
    person.check(person.lib.pbd_argmin_device_out(person.h, 0, after.data_ptr(), cap))
    person.check(person.lib.pbd_synchronize(person.h))
    assert torch.equal(before, after)
    assert np.array_equal(person.get_stage(_lib.STAGE_ROOTV, 1, 3, *stage.shape[1:]), stage)
    with pytest.raises(PbdError):
        person.boxes3d([depth.astype(np.int16)], [(480, 640)], rec[:1])
