"""Per-frame sort + non-maxima suppression on the device (pbd_set_nms, Handle.set_nms, PartsBasedDetector(nms=...)).

The yardstick is the Python mirror of the callers' post-step (cells/detect.cpp:237-238, ros/Node.cpp:192-196):
Candidate.sort(list) then Candidate.nonMaximaSuppression((rows, cols), list, float(np.float32(overlap))) on each frame's
candidates from the same handle with the stage off.  Every comparison is of int32 record arrays: same content, same order.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import Candidate, PbdError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAPS = (0.0, 0.1, 0.5, 1.0)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch's HIP runtime is initialised before this module creates its first handle (as the suite's earlier modules do)"""
    import torch
    torch.cuda.init()


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def mirror(rec: np.ndarray, rows: int, cols: int, overlap: float) -> np.ndarray:
    """rec: (n, stride) records of the stage-off list; returns the mirror's kept records, frame by frame"""
    keep = []
    for f in np.unique(rec[:, 0]):                       # ascending frame
        cands = []
        for i in np.nonzero(rec[:, 0] == f)[0]:
            r = rec[i]
            npart = int(r[6])
            conf = np.zeros(npart, np.float32)
            conf[0] = r[5:6].view(np.float32)[0]
            c = Candidate(parts=r[8:8 + 4 * npart].reshape(npart, 4), confidence=conf, component=int(r[1]), frame=int(f))
            c.row = int(i)
            cands.append(c)
        Candidate.sort(cands)
        Candidate.nonMaximaSuppression((rows, cols), cands, float(np.float32(overlap)))
        keep.extend(c.row for c in cands)
    return rec[np.array(keep, np.int64)] if keep else np.zeros((0, rec.shape[1]), np.int32)


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def _check_overlaps(hd, frames, min_per_frame=0):
    rows, cols = frames[0].shape[:2]
    hd.set_nms(None)
    raw = raw_batch(hd, frames)
    assert len(raw) >= min_per_frame * len(frames), len(raw)
    for ov in OVERLAPS:
        hd.set_nms(ov)
        got = raw_batch(hd, frames)
        want = mirror(raw, rows, cols, ov)
        assert got.shape == want.shape and np.array_equal(got, want), (ov, got.shape, want.shape)
    hd.set_nms(None)
    assert np.array_equal(raw_batch(hd, frames), raw)
    return raw


# ---- 1. real detections -------------------------------------------------------------------------------------------------
def test_person_batch64_640x480_lds_canvas():
    """the bench workload: person model, 64 synthetic 640x480 frames (bit canvas in LDS)"""
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=64)
    frames = [synth.synthetic_frame(i + 1, 480, 640, 3) for i in range(64)]
    raw = _check_overlaps(hd, frames, min_per_frame=20)
    assert len(np.unique(raw[:, 0])) > 32
    hd.close()


def test_person_8x1920x1080_global_canvas():
    """8 frames of 1920x1080: the bit canvas (259 KB) lives in the global workspace"""
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=8)
    frames = [synth.synthetic_frame(100 + i, 1080, 1920, 3) for i in range(8)]
    _check_overlaps(hd, frames, min_per_frame=20)
    hd.close()


def test_tiny_model_heavily_overlapping():
    hd = detector.Handle(M.synthetic_tiny_model(), device=0, max_batch=4)
    frames = [synth.synthetic_frame(7 + i, 240, 320, 3) for i in range(4)]
    raw = _check_overlaps(hd, frames, min_per_frame=100)
    # heavy overlap: suppression at 0.1 removes most of them
    hd.set_nms(0.1)
    assert len(raw_batch(hd, frames)) < len(raw) // 2
    hd.close()


# ---- 2. every entry point -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    model = M.synthetic_tiny_model(thresh=0.6)
    off = detector.PartsBasedDetector(device=0, max_batch=4)
    off.distributeModel(model)
    on = detector.PartsBasedDetector(device=0, max_batch=4, nms=0.1)
    on.distributeModel(model)
    batches = [[synth.synthetic_frame(31 * b + i + 1, 120, 150, 3) for i in range(4)] for b in range(3)]
    raws = [raw_batch(off.hd, fr) for fr in batches]
    assert all(len(r) > 8 for r in raws), [len(r) for r in raws]
    yield model, off, on, batches, raws
    off.hd.close()
    on.hd.close()


def _rec(det, buf, n):
    return np.array(buf[: n * det.hd.stride]).reshape(n, det.hd.stride)


def test_single_frame_entry_points(tiny):
    model, off, on, batches, raws = tiny
    im = batches[0][2]
    raw1 = raw_batch(off.hd, [im])
    want = mirror(raw1, 120, 150, 0.1)
    st = on.hd.stride
    buf = np.zeros(on.hd.max_candidates * st, np.int32)
    n = C.c_int()
    on.hd.check(on.hd.lib.pbd_detect(on.hd.h, im.ctypes.data, 120, 150, 3, 150 * 3, buf.ctypes.data, on.hd.max_candidates, C.byref(n)))
    assert np.array_equal(_rec(on, buf, n.value), want)
    on.hd.check(on.hd.lib.pbd_detect_typed(on.hd.h, im.ctypes.data, 120, 150, 3, 150 * 3, 0, buf.ctypes.data, on.hd.max_candidates,
                                           C.byref(n)))
    assert np.array_equal(_rec(on, buf, n.value), want)
    # a 16-bit image through pbd_detect_typed
    im16 = (im.astype(np.uint16) * 257)
    off16 = off.detect(im16)
    got16 = on.detect(im16)
    rec16 = np.zeros((len(off16), st), np.int32)
    for i, c in enumerate(off16):
        rec16[i, :5] = (c.frame, c.component, c.level, c.root[0], c.root[1])
        rec16[i, 5:6] = np.float32(c.score()).view(np.int32)
        rec16[i, 6] = len(c.parts)
        rec16[i, 8:8 + 4 * len(c.parts)] = c.parts.ravel()
    w16 = mirror(rec16, 120, 150, 0.1)
    assert [(c.component, c.level, c.root, c.parts.tobytes()) for c in got16] == \
        [(int(r[1]), int(r[2]), (int(r[3]), int(r[4])), r[8:8 + 4 * int(r[6])].tobytes()) for r in w16]


def test_batch_entry_points(tiny):
    import torch
    model, off, on, batches, raws = tiny
    wants = [mirror(r, 120, 150, 0.1) for r in raws]
    assert np.array_equal(raw_batch(on.hd, batches[0]), wants[0])
    dev = [torch.from_numpy(np.stack(fr)).cuda() for fr in batches]
    buf, n = on.detect_batch_device(dev[1].data_ptr(), 4, 120, 150, 3, raw=True)
    assert np.array_equal(_rec(on, buf, n), wants[1])
    # two batches in flight: host submit, then device submit
    on.submit_batch(batches[0])
    on.submit_batch_device(dev[2].data_ptr(), 4, 120, 150, 3)
    buf, n = on.wait_batch(raw=True)
    assert np.array_equal(_rec(on, buf, n), wants[0])
    buf, n = on.wait_batch(raw=True)
    assert np.array_equal(_rec(on, buf, n), wants[2])
    # the staged argmin (DynamicProgram::argmin) does not suppress
    feats = on.features_.pyramid(batches[0][0])
    resp = on.convolution_engine_.pdf(feats)
    on.dp_.min(resp)
    cands = on.dp_.argmin(on.features_.scales())
    assert len(cands) == int(np.sum(raw_batch(off.hd, batches[0][:1])[:, 0] == 0))


def test_device_out_payload_and_regrown_reemit(tiny):
    import torch
    model, off, on, batches, raws = tiny
    st = on.hd.stride
    want = mirror(raws[1], 120, 150, 0.1)
    shifted = want.copy()
    shifted[:, 0] += 500
    d = torch.from_numpy(np.stack(batches[1])).cuda()
    cap = len(want) + 5
    pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
    on.detect_batch_device_out(d.data_ptr(), 4, 120, 150, 3, 500, pay.data_ptr(), cap)
    on.hd.check(on.hd.lib.pbd_synchronize(on.hd.h))
    got = pay.cpu().numpy()
    assert got[0] == len(want)
    assert np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), shifted)
    assert np.all(got[1 + len(want) * st:] == -7)
    # overflow into a small payload: word 0 = kept count, the first `small` records present
    assert len(want) >= 2
    small = len(want) // 2
    pay2 = torch.full((1 + small * st,), -7, dtype=torch.int32, device="cuda")
    on.detect_batch_device_out(d.data_ptr(), 4, 120, 150, 3, 500, pay2.data_ptr(), small)
    on.hd.check(on.hd.lib.pbd_synchronize(on.hd.h))
    g2 = pay2.cpu().numpy()
    assert g2[0] == len(want)
    assert np.array_equal(g2[1:].reshape(small, st), shifted[:small])
    # grown re-emit without re-running the dynamic program
    pay3 = torch.full((1 + len(want) * st,), -7, dtype=torch.int32, device="cuda")
    on.argmin_device_out(500, pay3.data_ptr(), len(want))
    on.hd.check(on.hd.lib.pbd_synchronize(on.hd.h))
    g3 = pay3.cpu().numpy()
    assert g3[0] == len(want) and np.array_equal(g3[1:].reshape(-1, st), shifted)


def test_kept_count_over_caller_capacity_truncates(tiny):
    model, off, on, batches, raws = tiny
    on.hd.set_nms(1.0)                         # nothing suppressed: the kept list is the whole sorted list
    try:
        want = mirror(raws[0], 120, 150, 1.0)
        assert len(want) > 3
        with pytest.raises(PbdError) as e:
            on.detect_batch(batches[0], capacity=3)
        assert e.value.code == -4
        buf, n = np.zeros(3 * on.hd.stride, np.int32), C.c_int()
        fr = [np.ascontiguousarray(f) for f in batches[0]]
        rc = on.hd.lib.pbd_detect_batch(on.hd.h, 4, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, 3, C.byref(n))
        assert rc == -4 and n.value == 3
        assert np.array_equal(buf.reshape(3, -1), want[:3])
    finally:
        on.hd.set_nms(0.1)


@pytest.mark.parametrize("kind", ["double", "mfma"])
def test_double_and_mfma_handles(kind):
    if kind == "double":
        model, kw, shape, nf = M.synthetic_tiny_model(thresh=0.6), dict(real_type=_lib.REAL_F64), (120, 150), 4
    else:
        model, kw, shape, nf = M.synthetic_person_model(), dict(conv_mode=_lib.CONV_MFMA), (480, 640), 4
    hd = detector.Handle(model, device=0, max_batch=nf, **kw)
    frames = [synth.synthetic_frame(60 + i, shape[0], shape[1], 3) for i in range(nf)]
    _check_overlaps(hd, frames, min_per_frame=2)
    hd.close()


def test_detector_pool_with_nms(tiny):
    model, off, on, batches, raws = tiny
    pool = detector.DetectorPool(model, n=2, device=0, max_batch=4, nms=0.1)
    got = []
    for fr in batches:
        while pool.ready_before_next_submit:
            buf, n = pool.wait_batch(raw=True)
            got.append(np.array(buf[: n * on.hd.stride]).reshape(n, -1))
        pool.submit_batch(fr)
    while pool.pending:
        buf, n = pool.wait_batch(raw=True)
        got.append(np.array(buf[: n * on.hd.stride]).reshape(n, -1))
    assert len(got) == 3
    for g, r in zip(got, raws):
        assert np.array_equal(g, mirror(r, 120, 150, 0.1))
    pool.close()


_CHILD = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = str({port})
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from partsbaseddetector_amd import dist as pd, synth, detector
from partsbaseddetector_amd import model as M
from test_gpu_nms import mirror, raw_batch

model = M.synthetic_tiny_model(thresh=0.6)
off = detector.PartsBasedDetector(device=0, max_batch=4, max_candidates=1 << 14)
off.distributeModel(model)
det = detector.PartsBasedDetector(device=0, max_batch=4, max_candidates=1 << 14, nms=0.1)
det.distributeModel(model)
st = det.hd.stride
batches = [[synth.synthetic_frame(17 * b + i + 1, 120, 150, 3) for i in range(4)] for b in range(3)]
want = []
for b, fr in enumerate(batches):
    w = mirror(raw_batch(off.hd, fr), 120, 150, 0.1)
    w[:, 0] += 100 * b
    want.append(w)
dev = [torch.from_numpy(np.stack(fr)).cuda() for fr in batches]
g = pd.CandidateGatherer(st, cap=2, device="cuda:0", force_collective=True, cap_full=det.hd.max_candidates)
dg = pd.DeviceBatchGather(det, g)
outs = []
for b in range(3):
    prev = dg.submit(dev[b].data_ptr(), 4, 120, 150, 3, frame_offset=100 * b, root_only=True)
    if prev is not None:
        outs.append(prev)
outs.append(dg.collect(root_only=True))
res = {{"backend": dist.get_backend(), "world": dist.get_world_size(), "grown": g.grown,
        "ok": len(outs) == 3 and all(np.array_equal(o, w) for o, w in zip(outs, want)), "counts": [len(w) for w in want]}}
off.hd.close(); det.hd.close()
dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_rccl_world1_gathers_suppressed_payload(tmp_path):
    """fresh child process: torch.distributed 'nccl' at world size 1, DeviceBatchGather over suppressed device payloads"""
    import json
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, port=port))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["backend"] == "nccl" and res["world"] == 1
    assert res["ok"] and (res["grown"] >= 1) == (max(res["counts"]) > 2), res


# ---- 3. crafted lists through pbd_debug_postprocess ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def hd():
    h = detector.Handle(M.synthetic_tiny_model(), device=0, max_batch=1)
    yield h
    h.close()


def make(hd, frames, scores, boxes):
    """records with one part each (nparts 1) -- or the given part lists"""
    rec = np.zeros((len(scores), hd.stride), np.int32)
    for i, (f, s, b) in enumerate(zip(frames, scores, boxes)):
        parts = np.array(b, np.int32).reshape(-1, 4)
        rec[i, 0] = f
        rec[i, 2] = i            # level: distinguishes records that are otherwise alike
        rec[i, 5:6] = np.float32(s).view(np.int32)
        rec[i, 6] = len(parts)
        rec[i, 8:8 + parts.size] = parts.ravel()
    return rec


def post(hd, rec, rows, cols, overlap, capacity=None):
    cap = len(rec) if capacity is None else capacity
    out = np.zeros(max(cap, 1) * hd.stride, np.int32)
    n = C.c_int()
    src = np.ascontiguousarray(rec)
    hd.check(hd.lib.pbd_debug_postprocess(hd.h, rows, cols, src.ctypes.data, len(rec), overlap, out.ctypes.data, cap, C.byref(n)))
    return out[: n.value * hd.stride].reshape(n.value, hd.stride)


def check(hd, rec, rows, cols, overlap):
    got = post(hd, rec, rows, cols, overlap)
    want = mirror(rec, rows, cols, overlap)
    assert got.shape == want.shape and np.array_equal(got, want)
    return got


def test_exact_ties_keep_device_order(hd):
    rng = np.random.default_rng(5)
    n = 300
    scores = rng.choice(np.array([1.5, 0.25, -2.0], np.float32), n)
    boxes = [(int(x), int(y), 6, 6) for x, y in zip(rng.integers(0, 60, n), rng.integers(0, 40, n))]
    rec = make(hd, [0] * n, scores, boxes)
    for ov in (0.0, 0.3, 1.0):
        check(hd, rec, 48, 64, ov)
    # shuffled: the output follows the INPUT order among equal scores (stable), whatever that order is
    perm = rng.permutation(n)
    got = check(hd, rec[perm], 48, 64, 1.0)         # overlap 1.0: nothing is suppressed, the output is the sort
    assert len(got) == n
    for s in np.unique(scores):
        lv = got[got[:, 5].view(np.float32) == s][:, 2]
        pos = {int(lvl): k for k, lvl in enumerate(rec[perm][:, 2])}
        assert [pos[int(v)] for v in lv] == sorted(pos[int(v)] for v in lv)


def test_signed_zero_scores_tie(hd):
    rec = make(hd, [0, 0, 0, 0], [0.0, -0.0, 0.0, -0.0], [(0, 0, 4, 4)] * 4)
    got = check(hd, rec, 16, 16, 1.0)
    assert list(got[:, 2]) == [0, 1, 2, 3]
    rec = make(hd, [0, 0, 0], [-0.0, 1e-30, 0.0], [(0, 0, 4, 4), (8, 8, 4, 4), (0, 0, 4, 4)])
    check(hd, rec, 16, 16, 0.5)


def test_boxes_outside_and_covering_the_frame(hd):
    boxes = [(-5, -5, 10, 10),          # partly outside (top left)
             (30, 20, 50, 50),          # partly outside (bottom right)
             (100, 100, 5, 5),          # wholly outside: empty intersection -> kept
             (-20, 3, 10, 4),           # wholly outside on the left -> kept
             (0, 0, 40, 30),            # the whole frame
             (2, 2, 3, 3),
             (0, 0, 0, 5)]              # empty part
    rec = make(hd, [0] * len(boxes), [3, 2.5, 2, 1.5, 1, 0.5, 0.25], boxes)
    for ov in OVERLAPS:
        got = check(hd, rec, 30, 40, ov)
        assert set([2, 3, 6]) <= set(int(v) for v in got[:, 2])
    # multi-part hulls (the tiny model's records hold 3 parts) with empty parts in front and behind
    rec = make(hd, [0, 0], [1, 2], [[(0, 0, 0, 0), (3, 3, 4, 4), (10, 1, 2, 2)], [(9, 9, 0, 2), (1, 1, 2, 2), (5, 5, -1, 3)]])
    check(hd, rec, 20, 20, 0.0)


def test_ratio_between_double_and_float_tenth(hd):
    """a ratio r with 0.1 < r < (double)0.1f = 0.1 + 1.49e-9: kept, because the overlap is the reference's float widened"""
    W, H = 10001, 9999                       # A = 99 999 999 pixels; 10 000 000 of them painted: r = 0.1 + 1e-9
    assert 0.1 < 10_000_000 / (W * H) < float(np.float32(0.1))
    rec = make(hd, [0, 0, 0], [3, 2, 1], [(0, 0, W, 999), (0, 999, 9001, 1), (0, 0, W, H)])
    assert 999 * W + 9001 == 10_000_000
    got = check(hd, rec, H, W, 0.1)
    assert len(got) == 3
    # one pixel more: r > 0.1f -> suppressed
    rec = make(hd, [0, 0, 0], [3, 2, 1], [(0, 0, W, 999), (0, 999, 9002, 1), (0, 0, W, H)])
    assert len(check(hd, rec, H, W, 0.1)) == 2
    # the small exact case: 10 of 100 pixels, r = 0.1 (double) -> kept
    rec = make(hd, [0, 0], [2, 1], [(0, 0, 10, 1), (0, 0, 10, 10)])
    assert len(check(hd, rec, 16, 16, 0.1)) == 2


def test_twenty_thousand_candidates_in_one_frame(hd):
    rng = np.random.default_rng(11)
    n = 20000
    scores = rng.normal(size=n).astype(np.float32)
    scores[::7] = scores[3]                                   # plenty of ties as well
    xs, ys = rng.integers(-20, 640, n), rng.integers(-20, 480, n)
    ws, hs = rng.integers(1, 90, n), rng.integers(1, 120, n)
    rec = make(hd, [0] * n, scores, [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(xs, ys, ws, hs)])
    for ov in (0.1, 0.9):
        check(hd, rec, 480, 640, ov)
    check(hd, rec, 1080, 1920, 0.5)                           # the same list on the global-canvas path


def test_frames_with_zero_and_one_candidate(hd):
    rec = make(hd, [1, 3, 3, 3, 5], [1, 2, 3, 1, 7], [(0, 0, 8, 8), (0, 0, 8, 8), (1, 1, 8, 8), (20, 20, 4, 4), (2, 2, 2, 2)])
    for ov in OVERLAPS:
        got = check(hd, rec, 32, 32, ov)
        assert set(int(f) for f in got[:, 0]) == {1, 3, 5}
    assert len(post(hd, rec[:0], 32, 32, 0.1)) == 0
    one = check(hd, rec[:1], 32, 32, 0.0)
    assert len(one) == 1
    # the same multi-frame list on the global-canvas path
    check(hd, rec, 1200, 1200, 0.2)


def test_debug_entry_capacity_and_invalid_lists(hd):
    rec = make(hd, [0, 0, 0], [1, 2, 3], [(0, 0, 2, 2), (5, 5, 2, 2), (9, 9, 2, 2)])
    out = np.zeros(2 * hd.stride, np.int32)
    n = C.c_int()
    rc = hd.lib.pbd_debug_postprocess(hd.h, 16, 16, rec.ctypes.data, 3, 0.1, out.ctypes.data, 2, C.byref(n))
    assert rc == -4 and n.value == 2
    assert np.array_equal(out.reshape(2, -1), mirror(rec, 16, 16, 0.1)[:2])
    bad = rec[::-1].copy()
    bad[:, 0] = [2, 1, 0]                                     # frames not ascending
    assert hd.lib.pbd_debug_postprocess(hd.h, 16, 16, bad.ctypes.data, 3, 0.1, out.ctypes.data, 2, C.byref(n)) == -1
    bad = rec.copy()
    bad[1, 6] = 0                                             # no parts
    assert hd.lib.pbd_debug_postprocess(hd.h, 16, 16, bad.ctypes.data, 3, 0.1, out.ctypes.data, 2, C.byref(n)) == -1


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    model = M.synthetic_tiny_model(thresh=0.6)
    det = detector.PartsBasedDetector(device=0, max_batch=4)
    det.distributeModel(model)
    lib, h = det.hd.lib, det.hd.h
    assert lib.pbd_set_nms(h, 1, float("nan")) == -1
    frames = [synth.synthetic_frame(i + 1, 120, 150, 3) for i in range(4)]
    det.submit_batch(frames)
    assert lib.pbd_set_nms(h, 1, 0.1) == -5                   # latched at submit
    det.wait_batch()
    assert lib.pbd_set_nms(h, 1, 0.1) == 0
    assert lib.pbd_set_level_shard(h, 0, 2) == -2             # world > 1 while the stage is on
    assert lib.pbd_set_nms(h, 0, 0.1) == 0
    det.hd.set_level_shard(0, 2)
    assert lib.pbd_set_nms(h, 1, 0.1) == -2                   # and the other order
    det.hd.set_level_shard(0, 1)
    det.hd.close()


def test_found_over_max_candidates_is_refused_not_truncated():
    import torch
    model = M.synthetic_tiny_model()
    big = detector.Handle(model, device=0, max_batch=2)
    frames = [synth.synthetic_frame(i + 3, 120, 150, 3) for i in range(2)]
    found = len(raw_batch(big, frames))
    big.close()
    assert found > 20
    det = detector.PartsBasedDetector(device=0, max_batch=2, max_candidates=found - 5, nms=0.1)
    det.distributeModel(model)
    buf, n = np.zeros(found * det.hd.stride, np.int32), C.c_int(123)
    fr = [np.ascontiguousarray(f) for f in frames]
    rc = det.hd.lib.pbd_detect_batch(det.hd.h, 2, _lib.ptr_array(fr), 120, 150, 3, 450, buf.ctypes.data, found, C.byref(n))
    assert rc == -4 and n.value == 0
    assert "max_candidates" in det.hd.lib.pbd_last_error(det.hd.h).decode()
    det.submit_batch(frames)
    rc = det.hd.lib.pbd_detect_batch_wait(det.hd.h, buf.ctypes.data, found, C.byref(n))
    assert rc == -4 and n.value == 0
    st = det.hd.stride
    d = torch.from_numpy(np.stack(frames)).cuda()
    pay = torch.full((1 + found * st,), -7, dtype=torch.int32, device="cuda")
    det.detect_batch_device_out(d.data_ptr(), 2, 120, 150, 3, 0, pay.data_ptr(), found)
    det.hd.check(det.hd.lib.pbd_synchronize(det.hd.h))
    assert int(pay[0].item()) == -1
    det.hd.close()


# ---- 5. off by default --------------------------------------------------------------------------------------------------
def test_off_by_default_returns_the_raw_list(oracle):
    model = M.synthetic_tiny_model(thresh=0.6)
    fresh = detector.Handle(model, device=0, max_batch=1)
    im = synth.synthetic_frame(9, 120, 150, 3)
    raw = raw_batch(fresh, [im])
    want = oracle.detect(model.flatten(), im)
    assert len(raw) == len(want) and len(raw) > len(mirror(raw, 120, 150, 0.1))
    keys = [tuple(r[[0, 2, 1, 4, 3]]) for r in raw]
    assert keys == sorted(keys)
    fresh.set_nms(0.1)
    fresh.set_nms(None)
    assert np.array_equal(raw_batch(fresh, [im]), raw)
    fresh.close()
