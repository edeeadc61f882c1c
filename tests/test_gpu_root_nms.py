"""Root NMS on the detect path (pbd_set_root_nms, Handle.set_root_nms, PartsBasedDetector.setRootNMS).

The yardstick: the records of the same handle with the setting off, filtered by gridnms.grid_nms_ref(rootv plane, sz,
plane > thresh) at each record's (frame, level, component, root y, root x), where the planes are PBD_STAGE_ROOTV of that run.
Every comparison is of int32 record arrays: same content, same order.  The inputs' conditions (enough records, a real cut, not a
top-k) are checked on the CPU oracle in test_grid_nms_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, gridnms, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

from grid_nms_cases import ROOT_NMS_SIZES, ROOT_NMS_THRESH, root_nms_frames

pytestmark = pytest.mark.gpu
MIXED_SHAPES = ((120, 150), (100, 130), (140, 110))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def records(hd, frames):
    """the raw records of one call: pbd_detect_batch for equal sizes, pbd_detect_frames for mixed ones"""
    fr = [np.ascontiguousarray(f) for f in frames]
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    if len({f.shape for f in fr}) == 1:
        rows, cols, cn = fr[0].shape
        hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                         hd.max_candidates, C.byref(n)))
    else:
        descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
        hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


class Yardstick:
    """the records with the setting off and, per window size, their filtered list; the rootv planes are read once"""

    def __init__(self, hd, frames):
        hd.set_root_nms(0)
        self.raw = records(hd, frames)
        thr = hd.dtype(np.float32(hd.flat.thresh))
        self.planes, self.hit = {}, {}
        for f, im in enumerate(frames):
            pl = hd.plan(im.shape[0], im.shape[1])
            for l in range(pl["nlevels"]):
                r, c = int(pl["feat_rows"][l]), int(pl["feat_cols"][l])
                if r * c == 0:
                    continue
                rootv = hd.get_stage(_lib.STAGE_ROOTV, f, l, r, c)
                for comp in range(hd.flat.ncomponents):
                    self.planes[(f, l, comp)] = rootv[comp]
                    self.hit[(f, l, comp)] = rootv[comp] > thr
        self.kept = {}
        self.filtered = {}

    def want(self, sz):
        if sz not in self.filtered:
            self.kept[sz] = {k: gridnms.grid_nms_ref(p, sz, self.hit[k]) for k, p in self.planes.items()}
            self.filtered[sz] = gridnms.filter_records(self.raw, lambda f, l, c: self.kept[sz][(f, l, c)])
        return self.filtered[sz]


@pytest.fixture(scope="module")
def tiny():
    model = M.synthetic_tiny_model(thresh=ROOT_NMS_THRESH)
    det = detector.PartsBasedDetector(device=0, max_batch=4)
    det.distributeModel(model)
    hd = det.hd
    frames = root_nms_frames()
    mixed = [synth.synthetic_frame(41 + i, r, c, 3) for i, (r, c) in enumerate(MIXED_SHAPES)]
    ys = {"equal": Yardstick(hd, frames), "mixed": Yardstick(hd, mixed)}
    yield model, det, hd, {"equal": frames, "mixed": mixed}, ys
    hd.set_root_nms(0)
    hd.close()


@pytest.mark.parametrize("sz", ROOT_NMS_SIZES)
@pytest.mark.parametrize("kind", ["equal", "mixed"])
def test_records_equal_the_filtered_list(tiny, kind, sz):
    model, det, hd, frames, ys = tiny
    y = ys[kind]
    # every hit is a record of the unfiltered list, in (frame, level, component, y, x) order
    assert len(y.raw) == sum(int(h.sum()) for h in y.hit.values()) and len(y.raw) >= 50
    want = y.want(sz)
    assert 1 <= len(want) <= len(y.raw) // 2
    hd.set_root_nms(sz)
    try:
        got = records(hd, frames[kind])
    finally:
        hd.set_root_nms(0)
    assert got.shape == want.shape and np.array_equal(got, want)
    keys = [tuple(r[[0, 2, 1, 4, 3]]) for r in got]
    assert keys == sorted(keys)


@pytest.mark.parametrize("lanes", [1, 64])
def test_both_kernel_variants_on_the_detect_path(tiny, lanes):
    model, det, hd, frames, ys = tiny
    hd.set_debug_option(_lib.GRID_NMS_LANES, lanes)
    hd.set_root_nms(2)
    try:
        for kind in ("equal", "mixed"):
            assert np.array_equal(records(hd, frames[kind]), ys[kind].want(2))
    finally:
        hd.set_root_nms(0)
        hd.set_debug_option(_lib.GRID_NMS_LANES, 0)


def test_device_out_payloads(tiny):
    import torch
    model, det, hd, frames, ys = tiny
    st = hd.stride
    for sz in ROOT_NMS_SIZES:
        hd.set_root_nms(sz)
        try:
            for kind in ("equal", "mixed"):
                want = ys[kind].want(sz).copy()
                want[:, 0] += 300
                cap = len(want) + 3
                pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
                if kind == "equal":
                    d = torch.from_numpy(np.stack(frames[kind])).cuda()
                    det.detect_batch_device_out(d.data_ptr(), len(frames[kind]), 120, 150, 3, 300, pay.data_ptr(), cap)
                else:
                    ds = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames[kind]]
                    det.detect_frames_device_out([(t.data_ptr(), t.shape[0], t.shape[1], t.shape[1] * 3) for t in ds], 3, 300,
                                                 pay.data_ptr(), cap)
                hd.check(hd.lib.pbd_synchronize(hd.h))
                got = pay.cpu().numpy()
                assert got[0] == len(want)                                      # word 0: the kept count
                assert np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), want)
                assert np.all(got[1 + len(want) * st:] == -7)
            # the resident result re-emitted (pbd_argmin_device_out) goes through the step as well
            pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
            det.argmin_device_out(300, pay.data_ptr(), cap)
            hd.check(hd.lib.pbd_synchronize(hd.h))
            got = pay.cpu().numpy()
            assert got[0] == len(want) and np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), want)
        finally:
            hd.set_root_nms(0)


@pytest.mark.parametrize("kind", ["double", "three_components"])
def test_double_handle_and_three_components(kind):
    if kind == "double":
        model, kw = M.synthetic_tiny_model(thresh=ROOT_NMS_THRESH), dict(real_type=_lib.REAL_F64)
        frames = root_nms_frames()[:2]
    else:
        model, kw = M.synthetic_face_model(nparts=5, ncomponents=3, thresh=-100.0), {}     # every root cell passes the threshold
        frames = [synth.synthetic_frame(51 + i, 100, 120, 3) for i in range(2)]
    hd = detector.Handle(model, device=0, max_batch=2, **kw)
    try:
        y = Yardstick(hd, frames)
        assert len(y.raw) >= 50 and len({int(c) for c in y.raw[:, 1]}) == hd.flat.ncomponents
        for sz in ROOT_NMS_SIZES:
            hd.set_root_nms(sz)
            got = records(hd, frames)
            assert 1 <= len(got) < len(y.raw) and np.array_equal(got, y.want(sz)), (kind, sz)
    finally:
        hd.close()


def test_capacity_sees_only_the_kept_list(tiny):
    model, det, hd, frames, ys = tiny
    y = ys["equal"]
    found, kept = len(y.raw), len(y.want(2))
    cap = (found + kept) // 2
    assert kept < cap < found
    small = detector.Handle(model, device=0, max_batch=4, max_candidates=cap)
    try:
        fr = [np.ascontiguousarray(f) for f in frames["equal"]]
        buf, n = np.zeros(cap * small.stride, np.int32), C.c_int()
        args = (small.h, 4, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, cap, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4                      # off: more found than max_candidates
        small.set_root_nms(2)
        assert small.lib.pbd_detect_batch(*args) == 0 and n.value == kept
        assert np.array_equal(buf[: kept * small.stride].reshape(kept, -1), y.want(2))
        # the caller's capacity below the kept count: truncation and PBD_ERR_CAPACITY, as for any list
        args = (small.h, 4, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, kept - 1, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4 and n.value == kept - 1
        assert np.array_equal(buf[: (kept - 1) * small.stride].reshape(kept - 1, -1), y.want(2)[: kept - 1])
    finally:
        small.close()


def test_with_set_nms_the_result_is_suppress_of_the_filtered_list(tiny):
    model, det, hd, frames, ys = tiny
    for kind, shapes in (("equal", [(120, 150)] * 4), ("mixed", list(MIXED_SHAPES))):
        for sz in (1, 5):
            want = hd.suppress(shapes, 0.1, ys[kind].want(sz))
            hd.set_root_nms(sz)
            hd.set_nms(0.1)
            try:
                got = records(hd, frames[kind])
            finally:
                hd.set_nms(None)
                hd.set_root_nms(0)
            assert len(want) >= 1 and np.array_equal(got, want), (kind, sz)


def test_level_sharding_union_equals_the_unsharded_result(tiny):
    model, det, hd, frames, ys = tiny
    im = frames["equal"][1]
    want = ys["equal"].want(2)
    want = want[want[:, 0] == 1].copy()
    want[:, 0] = 0
    parts = []
    for rank in (0, 1):
        sh = detector.Handle(model, device=0, max_batch=1)
        try:
            sh.set_level_shard(rank, 2)
            sh.set_root_nms(2)
            parts.append(records(sh, [im]))
        finally:
            sh.close()
    assert all(len(p) for p in parts)
    union = np.concatenate(parts)
    union = union[np.lexsort((union[:, 3], union[:, 4], union[:, 1], union[:, 2]))]
    assert np.array_equal(union, want)


def test_latched_at_submit_and_refused_in_flight(tiny):
    model, det, hd, frames, ys = tiny
    det = detector.PartsBasedDetector(device=0, max_batch=4)
    det.setRootNMS(2)                                           # before distributeModel: kept across it
    det.distributeModel(model)
    try:
        det.submit_batch(frames["equal"])
        assert det.hd.lib.pbd_set_root_nms(det.hd.h, 0) == -5
        assert "waited" in det.hd.lib.pbd_last_error(det.hd.h).decode()
        buf, n = det.wait_batch(raw=True)
        assert np.array_equal(np.array(buf[: n * det.hd.stride]).reshape(n, -1), ys["equal"].want(2))
        det.setRootNMS(0)                                       # off again: the full list, bit for bit
        assert np.array_equal(records(det.hd, frames["equal"]), ys["equal"].raw)
        det.setRootNMS(5)
        det.distributeModel(model)                              # a new handle takes the setting over
        assert np.array_equal(records(det.hd, frames["equal"]), ys["equal"].want(5))
    finally:
        det.hd.close()


def test_detector_pool_forwards_the_setting(tiny):
    model, det, hd, frames, ys = tiny
    pool = detector.DetectorPool(model, n=2, device=0, max_batch=4)
    try:
        pool.setRootNMS(1)
        for _ in range(2):
            pool.submit_batch(frames["equal"])
        for _ in range(2):
            buf, n = pool.wait_batch(raw=True)
            assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), ys["equal"].want(1))
    finally:
        pool.close()


def test_dp_argmin_and_detect_latent_are_unaffected():
    model = M.synthetic_tiny_model(thresh=ROOT_NMS_THRESH)
    im = root_nms_frames()[0]
    det = detector.PartsBasedDetector(device=0, max_batch=1, max_candidates=1 << 16)
    det.distributeModel(model)
    try:
        full = det.detect(im)
        best = max(full, key=lambda c: c.score())
        boxes = [[(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts]]

        def run():
            det.dp_.min(det.convolution_engine_.pdf(det.features_.pyramid(im)))
            staged = det.hd.pack_candidates(det.dp_.argmin(det.features_.scales()))
            rec, found = det.hd.detect_latent([im], boxes, 0.3)
            return staged, rec.copy(), found.copy()
        off = run()
        det.setRootNMS(2)
        on = run()
        assert len(det.detect(im)) < len(full)                     # the setting is on for detect ...
        assert len(off[0]) == len(full) >= 50                       # ... and DynamicProgram::argmin still lists every root
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        assert off[2].all()
    finally:
        det.hd.close()


def test_refused_values(tiny):
    model, det, hd, frames, ys = tiny
    for sz in (-1, 32768, 1 << 20):
        assert hd.lib.pbd_set_root_nms(hd.h, sz) == -1
        assert "root NMS" in hd.lib.pbd_last_error(hd.h).decode()
    assert hd.lib.pbd_set_root_nms(hd.h, 32767) == 0 and hd.lib.pbd_set_root_nms(hd.h, 0) == 0
    det = detector.PartsBasedDetector(device=0)
    with pytest.raises(PbdError):
        det.setRootNMS(-2)
