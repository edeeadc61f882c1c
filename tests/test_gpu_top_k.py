"""The top-K selection on the GPU: the cells form (pbd_top_k_cells*), the detect path (pbd_set_top_k) and the list form
(pbd_top_k*), each against the numpy yardstick of topk.py, byte for byte and record for record.

Detect path: the yardstick is a list of the same handle with the setting off (the `base`), filtered by topk.top_k_cells_ref over
each frame's PBD_STAGE_ROOTV values in the find's order, where the cells of the base list are the eligible ones.  With root NMS or
depth pruning on, the base is the list those filters leave, so the check is also one of the filters' order.  The inputs'
conditions (a real cut, cuts inside ties) are checked on the CPU oracle in test_top_k_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth, topk
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

import top_k_cases as T
from top_k_cases import MIXED_SHAPES, TOP_K_SWEEP, TOP_K_THRESH, top_k_frames

pytestmark = pytest.mark.gpu
CASES = T.cases()
SENTINEL = 0x5A


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


class Planes:
    """every frame's rootv of the resident result in the find's order, (level, component, y, x), and where a cell lies in it"""

    def __init__(self, hd, frames):
        self.vals, self.where = [], {}
        for f, im in enumerate(frames):
            pl = hd.plan(im.shape[0], im.shape[1])
            parts, off = [], 0
            for l in range(pl["nlevels"]):
                r, c = int(pl["feat_rows"][l]), int(pl["feat_cols"][l])
                if r * c == 0:
                    continue
                rootv = hd.get_stage(_lib.STAGE_ROOTV, f, l, r, c)
                for comp in range(hd.flat.ncomponents):
                    self.where[(f, l, comp)] = (off, c)
                    parts.append(np.asarray(rootv[comp]).ravel())
                    off += r * c
            self.vals.append(np.concatenate(parts))

    def index(self, rec):
        """the place of every record's root cell in its frame's values"""
        out = np.zeros(len(rec), np.int64)
        for i, r in enumerate(rec):
            off, cols = self.where[(int(r[0]), int(r[2]), int(r[1]))]
            out[i] = off + int(r[4]) * cols + int(r[3])
        return out

    def top_k(self, base, k):
        """`base` filtered: per frame the k best of its records' cells"""
        idx = self.index(base)
        keep = np.zeros(len(base), bool)
        for f, v in enumerate(self.vals):
            mine = np.flatnonzero(base[:, 0] == f)
            mask = np.zeros(len(v), np.uint8)
            mask[idx[mine]] = 1
            keep[mine] = topk.top_k_cells_ref(v, k, mask)[idx[mine]] != 0
        return base[keep]


class Yardstick:
    def __init__(self, hd, frames):
        hd.set_top_k(0)
        self.raw = records(hd, frames)
        self.planes = Planes(hd, frames)
        self._want = {}

    def want(self, k):
        if k not in self._want:
            self._want[k] = self.planes.top_k(self.raw, k)
        return self._want[k]


def with_top_k(hd, k, frames):
    hd.set_top_k(k)
    try:
        return records(hd, frames)
    finally:
        hd.set_top_k(0)


@pytest.fixture(scope="module")
def tiny():
    model = M.synthetic_tiny_model(thresh=TOP_K_THRESH)
    det = detector.PartsBasedDetector(device=0, max_batch=4)
    det.distributeModel(model)
    hd = det.hd
    frames = top_k_frames()
    mixed = [synth.synthetic_frame(41 + i, r, c, 3) for i, (r, c) in enumerate(MIXED_SHAPES)]
    ys = {"equal": Yardstick(hd, frames), "mixed": Yardstick(hd, mixed)}
    yield model, det, hd, {"equal": frames, "mixed": mixed}, ys
    hd.set_top_k(0)
    hd.close()


# ---- the cells form ------------------------------------------------------------------------------------------------------------
def packed(case, dtype):
    vals, masks = case.values(dtype), case.mask_list()
    want = topk.top_k_segments_ref(vals, case.k, masks)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).ravel() for x in xs] or [np.zeros(0, dt)])
    return vals, masks, cat(vals, dtype), None if masks is None else cat(masks, np.uint8), cat(want, np.uint8)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cells_host_and_device_forms_equal_the_yardstick(tiny, case, dtype):
    import torch
    hd = tiny[2]
    vals, masks, src, msk, want = packed(case, dtype)
    got = hd.top_k_cells(vals, case.k, masks)
    assert np.array_equal(np.concatenate([g.ravel() for g in got]), want), case.name
    d_src = torch.from_numpy(src).cuda()
    d_msk = None if msk is None else torch.from_numpy(msk).cuda()                 # any non-zero byte counts
    outs = []
    for _ in range(2):                                                            # two runs: identical bytes
        d_dst = torch.full((len(src) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        hd.top_k_cells_device([len(v) for v in vals], _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64,
                              d_src.data_ptr() if len(src) else 0, None if d_msk is None else d_msk.data_ptr(), case.k,
                              d_dst.data_ptr())
        hd.check(hd.lib.pbd_synchronize(hd.h))
        outs.append(d_dst.cpu().numpy())
    assert np.array_equal(outs[0][: len(src)], want) and np.all(outs[0][len(src):] == SENTINEL)
    assert np.array_equal(outs[0], outs[1])


def test_cells_device_form_on_more_segments_than_the_grid(tiny):
    import torch
    hd = tiny[2]
    segs = [s.astype(np.float32) for s in T.many_segments()]
    want = np.concatenate(topk.top_k_segments_ref(segs, 2))
    src = np.concatenate(segs)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((len(src) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    hd.top_k_cells_device([len(s) for s in segs], _lib.REAL_F32, d_src.data_ptr(), None, 2, d_dst.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    got = d_dst.cpu().numpy()
    assert np.array_equal(got[: len(src)], want) and np.all(got[len(src):] == SENTINEL)


def test_cells_refusals(tiny):
    hd = tiny[2]
    lib, h = hd.lib, hd.h
    v = np.zeros(4, np.float32)
    d = np.zeros(4, np.uint8)
    ln = (C.c_longlong * 2)(2, 2)
    ok = lambda *a: lib.pbd_top_k_cells(h, *a)
    assert ok(2, ln, _lib.REAL_F32, v.ctypes.data, None, 1, d.ctypes.data) == 0
    assert ok(2, ln, _lib.REAL_F32, v.ctypes.data, None, -1, d.ctypes.data) == -1
    assert ok(-1, ln, _lib.REAL_F32, v.ctypes.data, None, 1, d.ctypes.data) == -1
    assert ok(2, ln, 7, v.ctypes.data, None, 1, d.ctypes.data) == -1
    assert ok(2, None, _lib.REAL_F32, v.ctypes.data, None, 1, d.ctypes.data) == -1
    assert ok(2, ln, _lib.REAL_F32, None, None, 1, d.ctypes.data) == -1
    assert ok(2, ln, _lib.REAL_F32, v.ctypes.data, None, 1, None) == -1
    assert ok(2, (C.c_longlong * 2)(2, -2), _lib.REAL_F32, v.ctypes.data, None, 1, d.ctypes.data) == -1
    assert ok(2, (C.c_longlong * 2)(1 << 30, 1 << 30), _lib.REAL_F32, v.ctypes.data, None, 1, d.ctypes.data) == -1   # 2^31 in all
    assert ok(2, (C.c_longlong * 2)(0, 0), _lib.REAL_F32, None, None, 1, None) == 0                # nothing to do
    assert ok(0, None, _lib.REAL_F64, None, None, 0, None) == 0
    assert lib.pbd_top_k_cells_device(h, 2, ln, _lib.REAL_F32, None, None, 1, None) == -1


# ---- the detect path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", TOP_K_SWEEP)
@pytest.mark.parametrize("kind", ["equal", "mixed"])
def test_records_equal_the_filtered_list(tiny, kind, k):
    model, det, hd, frames, ys = tiny
    y = ys[kind]
    nfr = len(frames[kind])
    per_frame = np.bincount(y.raw[:, 0], minlength=nfr)
    assert len(y.raw) >= 50
    want = y.want(k)
    assert np.array_equal(np.bincount(want[:, 0], minlength=nfr), np.minimum(per_frame, k))
    got = with_top_k(hd, k, frames[kind])
    assert got.shape == want.shape and np.array_equal(got, want)
    keys = [tuple(r[[0, 2, 1, 4, 3]]) for r in got]
    assert keys == sorted(keys)
    if k < per_frame.max():
        assert len(got) < len(y.raw)


def test_threshold_at_zero_cuts_inside_long_runs(tiny):
    """the constant frame's root scores come in a few hundred values: K cuts inside runs of hundreds of equal cells"""
    model, det, hd, frames, ys = tiny
    hd.set_thresh(0.0)
    try:
        y = Yardstick(hd, frames["equal"])
        grey = y.raw[y.raw[:, 0] == 3]
        assert len(grey) > 1000 and len(np.unique(grey[:, 5])) < len(grey) // 4
        for k in TOP_K_SWEEP:
            assert np.array_equal(with_top_k(hd, k, frames["equal"]), y.want(k)), k
    finally:
        hd.set_thresh(TOP_K_THRESH)


def test_double_handle():
    model = M.synthetic_tiny_model(thresh=TOP_K_THRESH)
    hd = detector.Handle(model, device=0, max_batch=2, real_type=_lib.REAL_F64)
    try:
        frames = top_k_frames()[:2]
        y = Yardstick(hd, frames)
        assert y.planes.vals[0].dtype == np.float64 and len(y.raw) >= 50
        for k in TOP_K_SWEEP:
            assert np.array_equal(with_top_k(hd, k, frames), y.want(k)), k
    finally:
        hd.close()


@pytest.mark.parametrize("kind", ["equal", "mixed"])
def test_after_root_nms_k_is_taken_among_the_maxima(tiny, kind):
    model, det, hd, frames, ys = tiny
    hd.set_root_nms(2)
    try:
        base = records(hd, frames[kind])
        assert 10 <= len(base) < len(ys[kind].raw)
        for k in (1, 2, 5, 64):
            want = ys[kind].planes.top_k(base, k)
            got = with_top_k(hd, k, frames[kind])
            assert np.array_equal(got, want), k
            if k == 64:
                assert not np.array_equal(got, ys[kind].want(k))            # not the K best of all roots: those hold neighbours
    finally:
        hd.set_root_nms(0)


def test_after_depth_pruning_k_is_taken_among_the_plausible(tiny):
    model, det, hd, frames, ys = tiny
    y = ys["equal"]
    # depth images in which a root box 40 units wide is plausible at half of the widths the list holds
    widths = sorted({int(w) for w in y.raw[:, 10]})
    rng = np.random.default_rng(3)
    vals = np.rint(np.array([500.0 * 40.0 / w for w in widths[::2]]))
    depths = [vals[np.kron(rng.integers(0, len(vals), (24, 30)), np.ones((5, 5), np.int64))].astype(np.uint16) for _ in range(4)]
    hd.set_depth_prune(500.0, 40.0, 0.02)
    try:
        hd.bind_depth(depths)
        base = records(hd, frames["equal"])
        assert 10 <= len(base) < len(y.raw)
        for k in (1, 5, 64):
            hd.bind_depth(depths)
            assert np.array_equal(with_top_k(hd, k, frames["equal"]), y.planes.top_k(base, k)), k
        # all three filters: pruning, then the grid maxima among the plausible, then K among those
        hd.set_root_nms(2)
        hd.bind_depth(depths)
        base = records(hd, frames["equal"])
        hd.bind_depth(depths)
        assert np.array_equal(with_top_k(hd, 3, frames["equal"]), y.planes.top_k(base, 3))
    finally:
        hd.set_root_nms(0)
        hd.set_depth_prune(None)


def test_device_out_payloads_and_re_emission_under_another_k(tiny):
    import torch
    model, det, hd, frames, ys = tiny
    st = hd.stride
    for kind in ("equal", "mixed"):
        hd.set_top_k(5)
        try:
            want = ys[kind].want(5).copy()
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
            # the resident result re-emitted under a second K, without a new detect call
            hd.set_top_k(2)
            want = ys[kind].want(2).copy()
            want[:, 0] += 300
            pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
            det.argmin_device_out(300, pay.data_ptr(), cap)
            hd.check(hd.lib.pbd_synchronize(hd.h))
            got = pay.cpu().numpy()
            assert got[0] == len(want) and np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), want)
        finally:
            hd.set_top_k(0)


def test_with_set_nms_the_result_is_suppress_of_the_kept_list(tiny):
    model, det, hd, frames, ys = tiny
    for kind, shapes in (("equal", [(120, 150)] * 4), ("mixed", list(MIXED_SHAPES))):
        for k in (5, 64):
            want = hd.suppress(shapes, 0.1, ys[kind].want(k))
            hd.set_nms(0.1)
            try:
                got = with_top_k(hd, k, frames[kind])
            finally:
                hd.set_nms(None)
            assert 1 <= len(want) <= len(ys[kind].want(k)) and np.array_equal(got, want), (kind, k)


def test_capacity_and_a_threshold_free_run(tiny, oracle):
    """thresh = -inf lists every root: more than max_candidates without K, exactly K per frame with it"""
    model, det, hd, frames, ys = tiny
    small = detector.Handle(model, device=0, max_batch=4, max_candidates=1000)
    try:
        small.set_thresh(-np.inf)
        fr = [np.ascontiguousarray(f) for f in frames["equal"]]
        buf, n = np.zeros(1000 * small.stride, np.int32), C.c_int()
        args = (small.h, 4, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, 1000, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4                      # off: more found than max_candidates
        small.set_top_k(100)
        assert small.lib.pbd_detect_batch(*args) == 0 and n.value == 400
        got = buf[: 400 * small.stride].reshape(400, -1).copy()
        assert np.array_equal(np.bincount(got[:, 0]), [100] * 4)
        planes = Planes(small, frames["equal"])
        idx = planes.index(got)
        for f, v in enumerate(planes.vals):
            want = np.flatnonzero(topk.top_k_cells_ref(v, 100, v > -np.inf))
            assert np.array_equal(idx[got[:, 0] == f], want), f
        # frame 0 against the CPU oracle's planes
        v = T.oracle_frame_values(oracle, model.flatten(), frames["equal"][0])
        assert np.array_equal(idx[got[:, 0] == 0], np.flatnonzero(topk.top_k_cells_ref(v, 100, v > -np.inf)))
        # the caller's capacity below the kept count: truncation and PBD_ERR_CAPACITY, as for any list
        args = (small.h, 4, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, 399, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4 and n.value == 399
        assert np.array_equal(buf[: 399 * small.stride].reshape(399, -1), got[:399])
    finally:
        small.close()


def test_level_shards_merged_and_reselected_equal_the_unsharded_result(tiny):
    model, det, hd, frames, ys = tiny
    im = frames["equal"][1]
    for k in (2, 5, 64):
        want = ys["equal"].want(k)
        want = want[want[:, 0] == 1].copy()
        want[:, 0] = 0
        parts = []
        for rank in (0, 1):
            sh = detector.Handle(model, device=0, max_batch=1)
            try:
                sh.set_level_shard(rank, 2)
                sh.set_top_k(k)
                parts.append(records(sh, [im]))
            finally:
                sh.close()
        assert all(1 <= len(p) <= k for p in parts) and sum(len(p) for p in parts) > len(want)
        merged = topk.canonical_order(np.concatenate(parts))
        assert {tuple(r) for r in want} <= {tuple(r) for r in merged}
        assert np.array_equal(hd.top_k(1, k, merged), want), k


def test_latched_at_submit_refused_in_flight_and_off_again(tiny):
    model, det, hd, frames, ys = tiny
    det = detector.PartsBasedDetector(device=0, max_batch=4)
    det.setTopK(5)                                              # before distributeModel: kept across it
    det.distributeModel(model)
    try:
        det.submit_batch(frames["equal"])
        assert det.hd.lib.pbd_set_top_k(det.hd.h, 0) == -5
        assert "waited" in det.hd.lib.pbd_last_error(det.hd.h).decode()
        v = np.zeros(4, np.float32)
        assert det.hd.lib.pbd_top_k_cells(det.hd.h, 1, (C.c_longlong * 1)(4), _lib.REAL_F32, v.ctypes.data, None, 1,
                                          np.zeros(4, np.uint8).ctypes.data) == -5
        assert det.hd.lib.pbd_top_k(det.hd.h, 1, 1, None, 0, 0, None, 0, C.byref(C.c_int())) == -5
        buf, n = det.wait_batch(raw=True)
        assert np.array_equal(np.array(buf[: n * det.hd.stride]).reshape(n, -1), ys["equal"].want(5))
        det.setTopK(0)                                          # off again: the full list, bit for bit
        assert np.array_equal(records(det.hd, frames["equal"]), ys["equal"].raw)
        det.setTopK(2)
        det.distributeModel(model)                              # a new handle takes the setting over
        assert np.array_equal(records(det.hd, frames["equal"]), ys["equal"].want(2))
        assert len(det.topK(det.detect(frames["equal"][0]), 1)) == 1
    finally:
        det.hd.close()


def test_detector_pool_forwards_the_setting(tiny):
    model, det, hd, frames, ys = tiny
    pool = detector.DetectorPool(model, n=2, device=0, max_batch=4)
    try:
        pool.setTopK(5)
        for _ in range(2):
            pool.submit_batch(frames["equal"])
        for _ in range(2):
            buf, n = pool.wait_batch(raw=True)
            assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), ys["equal"].want(5))
    finally:
        pool.close()


def test_dp_argmin_and_detect_latent_are_unaffected():
    model = M.synthetic_tiny_model(thresh=TOP_K_THRESH)
    im = top_k_frames()[0]
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
        det.setTopK(3)
        on = run()
        assert len(det.detect(im)) == 3 < len(full)                 # the setting is on for detect ...
        assert len(off[0]) == len(full) >= 50                       # ... and DynamicProgram::argmin still lists every root
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        assert off[2].all()
    finally:
        det.hd.close()


def test_refused_values(tiny):
    model, det, hd, frames, ys = tiny
    for k in (-1, (1 << 30) + 1, -(1 << 31)):
        assert hd.lib.pbd_set_top_k(hd.h, k) == -1
        assert "top-K" in hd.lib.pbd_last_error(hd.h).decode()
    assert hd.lib.pbd_set_top_k(hd.h, 1 << 30) == 0 and hd.lib.pbd_set_top_k(hd.h, 0) == 0
    det = detector.PartsBasedDetector(device=0)
    with pytest.raises(PbdError):
        det.setTopK(-2)


# ---- the list form -------------------------------------------------------------------------------------------------------------
def device_top_k(hd, nframes, k, rec, frame_offset=0, word0=None, out_cap=None):
    """pbd_top_k_device on a payload of the records; returns the output payload"""
    import torch
    st = hd.stride
    cap = max(len(rec), 1)
    pay = np.zeros(1 + cap * st, np.int32)
    pay[0] = len(rec) if word0 is None else word0
    pay[1:1 + rec.size] = rec.ravel()
    out_cap = cap if out_cap is None else out_cap
    d_in = torch.from_numpy(pay).cuda()
    d_out = torch.full((1 + max(out_cap, 1) * st,), -7, dtype=torch.int32, device="cuda")
    hd.top_k_device(nframes, k, d_in.data_ptr(), cap, frame_offset, d_out.data_ptr(), out_cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return d_out.cpu().numpy()


@pytest.mark.parametrize("case", T.RECORD_CASES, ids=[c[0] for c in T.RECORD_CASES])
def test_list_host_and_device_forms(tiny, case):
    hd = tiny[2]
    name, scores, k, _ = case
    st = hd.stride
    nframes = max(scores) + 1
    for off in (0, 300):
        rec = T.record_list(st, scores, off)
        want = topk.top_k_records_ref(rec, k)
        assert np.array_equal(hd.top_k(nframes, k, rec, off), want)
        got = device_top_k(hd, nframes, k, rec, off)
        assert got[0] == len(want) and np.array_equal(got[1:1 + want.size].reshape(-1, st), want)
        assert np.all(got[1 + want.size:] == -7)


@pytest.mark.parametrize("n", T.RECORD_COUNTS)
def test_list_sizes_and_in_place(tiny, n):
    hd = tiny[2]
    st = hd.stride
    rec = T.random_records(st, n, 7, 100 + n) if n else np.zeros((0, st), np.int32)
    for k in (0, 1, 40, 10000):
        want = topk.top_k_records_ref(rec, k)
        buf = rec.copy() if n else np.zeros((1, st), np.int32)
        kept = C.c_int(-3)
        assert hd.lib.pbd_top_k(hd.h, 7, k, buf.ctypes.data if n else None, n, 0, buf.ctypes.data if n else None, n,
                                C.byref(kept)) == 0                                        # in place
        assert kept.value == len(want) and np.array_equal(buf[: len(want)], want)
        got = device_top_k(hd, 7, k, rec)
        assert got[0] == len(want) and np.array_equal(got[1:1 + want.size].reshape(-1, st), want)


def test_list_word_0_conventions_and_refusals(tiny):
    hd = tiny[2]
    st = hd.stride
    rec = T.record_list(st, {0: [3, 1, 2], 1: [5, 4]})
    for word0 in (-1, -4, 6):                       # a status, or more than the capacity: no complete list
        got = device_top_k(hd, 2, 1, rec, word0=word0)
        assert got[0] == -1 and np.all(got[1:] == -7)
    got = device_top_k(hd, 2, 2, rec, out_cap=3)    # the kept count may exceed the capacity: the first three are written
    assert got[0] == 4 and np.array_equal(got[1:1 + 3 * st].reshape(-1, st), rec[[0, 2, 3]])
    kept = C.c_int()
    out = np.zeros((5, st), np.int32)
    call = lambda nframes, k, r, off=0: hd.lib.pbd_top_k(hd.h, nframes, k, r.ctypes.data, len(r), off, out.ctypes.data, 5, C.byref(kept))
    assert call(2, 1, rec) == 0 and kept.value == 2
    assert call(2, -1, rec) == -1 and call(0, 1, rec) == -1
    assert call(1, 1, rec) == -1                    # a frame outside 0 .. nframes - 1
    assert call(2, 1, rec[::-1].copy()) == -1       # frames not ascending
    bad = rec.copy(); bad[1, 6] = 0
    assert call(2, 1, bad) == -1                    # nparts outside 1..max parts
    # the device form drops such records, and they are nobody's rival
    bad = rec.copy(); bad[0, 6] = 0                 # the best record of frame 0
    got = device_top_k(hd, 2, 1, bad)
    assert got[0] == 2 and np.array_equal(got[1:1 + 2 * st].reshape(-1, st), rec[[2, 3]])
    got = device_top_k(hd, 1, 5, rec)               # frame 1 is outside the call's one frame
    assert got[0] == 3 and np.array_equal(got[1:1 + 3 * st].reshape(-1, st), rec[:3])
    assert hd.lib.pbd_top_k_device(hd.h, 2, -1, 8, 1, 0, 8, 1) == -1
