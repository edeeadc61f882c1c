"""Frames of different sizes in one call (pbd_detect_frames, _device, _device_out; PartsBasedDetector.detect_batch /
detect_frames / detect_regions; DeviceBatchGather.submit_frames).

The yardstick is the per-frame call on the same kind of handle: the records of a mixed call are those of one
pbd_detect_typed per frame, concatenated, with `frame` = index in the call.  Every comparison is of int32 record arrays.
"""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import Candidate, PbdError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 18


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def handle(model, **kw):
    kw.setdefault("max_batch", 16)
    kw.setdefault("max_candidates", CAP)
    return detector.Handle(model, **kw)


def records(hd, buf, n):
    return buf[: n * hd.stride].reshape(n, hd.stride).copy()


def depth_of(im):
    return _lib.DEPTH_CODE[im.dtype]


def hwc(im):
    return np.ascontiguousarray(im if im.ndim == 3 else im[:, :, None])


def single(hd, frames):
    """one pbd_detect_typed per frame, `frame` = index in the list, concatenated"""
    out = []
    for i, im in enumerate(frames):
        im = hwc(im)
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        n = C.c_int()
        hd.check(hd.lib.pbd_detect_typed(hd.h, im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], im.strides[0],
                                         depth_of(im), buf.ctypes.data, hd.max_candidates, C.byref(n)))
        r = records(hd, buf, n.value)
        r[:, 0] = i
        out.append(r)
    return np.concatenate(out) if out else np.zeros((0, hd.stride), np.int32)


def frames_call(hd, frames, capacity=None, allow=()):
    fr = [hwc(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    cap = capacity if capacity is not None else hd.max_candidates
    buf = np.zeros(max(cap, 1) * hd.stride, np.int32)
    n = C.c_int()
    rc = hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], depth_of(fr[0]), buf.ctypes.data, cap,
                                           C.byref(n)), allow)
    return (records(hd, buf, n.value), rc) if allow else records(hd, buf, n.value)


def mixed_sizes(seed, sizes, cn=3):
    return [synth.synthetic_frame(seed + i, r, c, cn) for i, (r, c) in enumerate(sizes)]


PERSON_MIX = [(1080, 1920), (720, 1280), (480, 640), (480, 640), (480, 640), (240, 320), (240, 320), (157, 201)]
SMALL_MIX = [(160, 200), (96, 128), (121, 157), (100, 100)]


# ---- 1. equal sizes: byte-identical to pbd_detect_batch -------------------------------------------------------------------
def test_equal_frames_match_detect_batch():
    hd = handle(M.synthetic_person_model(), max_batch=8)
    frames = [synth.synthetic_frame(100 + i, 480, 640, 3) for i in range(8)]
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, 8, _lib.ptr_array(frames), 480, 640, 3, 640 * 3, buf.ctypes.data, hd.max_candidates,
                                     C.byref(n)))
    want = records(hd, buf, n.value)
    got = frames_call(hd, frames)
    assert len(want) > 0
    assert got.tobytes() == want.tobytes()
    hd.close()


# ---- 2. mixed person call equals per-frame calls; tiny model equals the oracle --------------------------------------------
def test_mixed_person_equals_per_frame():
    hd = handle(M.synthetic_person_model())
    frames = mixed_sizes(200, PERSON_MIX)
    got = frames_call(hd, frames)
    want = single(hd, frames)
    assert len(want) > 0
    assert got.shape == want.shape and np.array_equal(got, want)
    hd.close()


def test_mixed_tiny_equals_oracle(oracle):
    model = M.synthetic_tiny_model(thresh=0.6)
    det = detector.PartsBasedDetector(max_batch=8, max_candidates=CAP)
    det.distributeModel(model)
    frames = mixed_sizes(300, [(96, 128), (120, 150), (80, 100), (133, 97)])
    got = det.detect_batch(frames)            # shapes differ: pbd_detect_frames
    flat = model.flatten()
    n = 0
    for f, im in enumerate(frames):
        want = oracle.detect(flat, im)
        mine = [c for c in got if c.frame == f]
        assert len(mine) == len(want)
        for g, w in zip(mine, want):
            assert (g.level, g.component, g.root[1], g.root[0]) == (w["level"], w["component"], w["root_y"], w["root_x"])
            assert np.array_equal(g.parts, w["parts"])
            assert np.float32(g.score()) == np.float32(w["score"])
        n += len(want)
    assert n == len(got) and n > 0


# ---- 3. staged read-back addresses (frame, level of that frame's pyramid) ---------------------------------------------------
def test_stages_and_pyramid_images_per_frame():
    model = M.synthetic_tiny_model(thresh=0.6)
    hd = handle(model)
    frames = mixed_sizes(400, SMALL_MIX)
    frames_call(hd, frames)
    mixed = {}
    for f, im in enumerate(frames):
        p = hd.plan(im.shape[0], im.shape[1])
        for l in range(p["nlevels"]):
            r, c = int(p["feat_rows"][l]), int(p["feat_cols"][l])
            img = np.empty((int(p["img_rows"][l]), int(p["img_cols"][l]), 3), np.uint8)
            hd.check(hd.lib.pbd_get_pyramid_image(hd.h, f, l, img.ctypes.data))
            st = [hd.get_stage(s, f, l, r, c) for s in (_lib.STAGE_FEATURES, _lib.STAGE_RESPONSES, _lib.STAGE_ROOTV)]
            mixed[f, l] = (img, st)
        with pytest.raises(PbdError):
            hd.get_stage(_lib.STAGE_FEATURES, f, p["nlevels"], 1, 1)
    for f, im in enumerate(frames):
        single(hd, [im])
        p = hd.plan(im.shape[0], im.shape[1])
        for l in range(p["nlevels"]):
            r, c = int(p["feat_rows"][l]), int(p["feat_cols"][l])
            img = np.empty_like(mixed[f, l][0])
            hd.check(hd.lib.pbd_get_pyramid_image(hd.h, 0, l, img.ctypes.data))
            assert np.array_equal(img, mixed[f, l][0]), (f, l)
            for s, want in zip((_lib.STAGE_FEATURES, _lib.STAGE_RESPONSES, _lib.STAGE_ROOTV), mixed[f, l][1]):
                assert hd.get_stage(s, 0, l, r, c).tobytes() == want.tobytes(), (f, l, s)
    hd.close()


# ---- 4. both real types, every conv mode, depths -----------------------------------------------------------------------------
@pytest.mark.parametrize("real,mode", [(_lib.REAL_F32, _lib.CONV_EXACT), (_lib.REAL_F32, _lib.CONV_FMA),
                                       (_lib.REAL_F32, _lib.CONV_MFMA), (_lib.REAL_F32, _lib.CONV_MFMA_F16),
                                       (_lib.REAL_F64, _lib.CONV_EXACT), (_lib.REAL_F64, _lib.CONV_FMA),
                                       (_lib.REAL_F64, _lib.CONV_MFMA_F64)])
def test_every_mode_equals_per_frame(real, mode):
    hd = handle(M.synthetic_person_model(thresh=0.0), real_type=real, conv_mode=mode)
    frames = mixed_sizes(500, [(160, 200), (121, 157), (96, 128)])
    got = frames_call(hd, frames)
    want = single(hd, frames)
    assert len(want) > 0
    assert np.array_equal(got, want)
    hd.close()


def test_grey_and_float_frames():
    hd = handle(M.synthetic_tiny_model(thresh=0.3))
    grey = mixed_sizes(600, SMALL_MIX, cn=1)
    got = frames_call(hd, grey)
    assert len(got) > 0 and np.array_equal(got, single(hd, grey))
    flt = [f.astype(np.float32) * np.float32(0.7) for f in mixed_sizes(700, SMALL_MIX)]
    want = single(hd, flt)
    got = frames_call(hd, flt)                   # the mixed result stays resident through the refusal below
    assert len(got) > 0 and np.array_equal(got, want)
    p = hd.plan(*SMALL_MIX[0])
    shape = (int(p["feat_rows"][0]), int(p["feat_cols"][0]))
    before = hd.get_stage(_lib.STAGE_ROOTV, 0, 0, *shape)
    flt[2][5, 7, 1] = np.nan
    with pytest.raises(PbdError, match="frame 2"):
        frames_call(hd, flt)
    assert hd.get_stage(_lib.STAGE_ROOTV, 0, 0, *shape).tobytes() == before.tobytes()
    hd.close()


# ---- 5. regions of one device image -----------------------------------------------------------------------------------------
def test_regions_read_in_place():
    import torch
    model = M.synthetic_tiny_model(thresh=0.4)
    det = detector.PartsBasedDetector(max_batch=8, max_candidates=CAP)
    det.distributeModel(model)
    hd = det.hd
    H, W, PW = 300, 400, 416
    img = synth.synthetic_frame(800, H, W, 3)
    # rows PW*3 bytes apart (pitch != width), and the storage ends with the image's last pixel: no byte after it
    pitch = PW * 3
    store = torch.zeros((H - 1) * pitch + W * 3, dtype=torch.uint8, device="cuda")
    dev = torch.as_strided(store, (H, W, 3), (pitch, 3, 1))
    dev.copy_(torch.from_numpy(img).cuda())
    assert dev.stride(0) == pitch and dev[H - 1, W - 1, 2].data_ptr() == store.data_ptr() + store.numel() - 1
    rects = [(0, 0, 200, 150), (37, 41, 160, 120), (W - 150, H - 130, 150, 130), (100, 100, 96, 128)]   # #2 ends at the last pixel
    crops = [np.ascontiguousarray(img[y:y + h, x:x + w]) for x, y, w, h in rects]
    want = frames_call(hd, crops)
    assert len(want) > 0
    descs = _lib.frame_array([(dev.data_ptr() + y * pitch + x * 3, h, w, pitch) for x, y, w, h in rects])
    torch.cuda.synchronize()
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames_device(hd.h, len(rects), descs, 3, 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    assert np.array_equal(records(hd, buf, n.value), want)
    got = det.detect_regions(dev, rects)
    assert len(got) == len(want)
    for c, r in zip(got, want):
        assert (c.frame, c.level, c.component, c.root[0], c.root[1]) == (r[0], r[2], r[1], r[3], r[4])
        assert np.array_equal(c.parts.ravel(), r[8:8 + 4 * int(r[6])])
        assert c.offset == rects[c.frame][:2]


# ---- 6. device-out payload, overflow, re-emit --------------------------------------------------------------------------------
def test_device_out_offset_overflow_reemit():
    import torch
    hd = handle(M.synthetic_tiny_model(thresh=0.4))
    frames = mixed_sizes(900, SMALL_MIX)
    want = frames_call(hd, frames)
    assert len(want) > 2
    dev = [torch.from_numpy(f).cuda() for f in frames]
    descs = _lib.frame_array([(d.data_ptr(), d.shape[0], d.shape[1], d.stride(0)) for d in dev])
    torch.cuda.synchronize()
    small = len(want) // 2
    pay = torch.zeros(1 + small * hd.stride, dtype=torch.int32, device="cuda")
    hd.check(hd.lib.pbd_detect_frames_device_out(hd.h, len(frames), descs, 3, 0, 7, pay.data_ptr(), small))
    hd.check(hd.lib.pbd_synchronize(hd.h))
    p = pay.cpu().numpy()
    assert p[0] == len(want)
    shifted = want.copy()
    shifted[:, 0] += 7
    assert np.array_equal(p[1:].reshape(small, hd.stride), shifted[:small])
    big = torch.zeros(1 + len(want) * hd.stride, dtype=torch.int32, device="cuda")
    hd.check(hd.lib.pbd_argmin_device_out(hd.h, 7, big.data_ptr(), len(want)))
    hd.check(hd.lib.pbd_synchronize(hd.h))
    b = big.cpu().numpy()
    assert b[0] == len(want) and np.array_equal(b[1:].reshape(len(want), hd.stride), shifted)
    hd.close()


# ---- 7. non-maxima suppression, both canvas kinds in one call -------------------------------------------------------------
def mirror(rec, sizes, overlap):
    keep = []
    for f in np.unique(rec[:, 0]):
        rows, cols = sizes[int(f)]
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


def test_nms_per_frame_with_both_canvas_kinds():
    hd = handle(M.synthetic_person_model())
    sizes = [(480, 640), (1080, 1920), (480, 640), (157, 201)]     # 1080p: 259 KB canvas (global); the others fit LDS
    frames = mixed_sizes(1000, sizes)
    raw = frames_call(hd, frames)
    assert len(raw) > 0 and (raw[:, 0] == 1).any()
    for ov in (0.0, 0.1, 0.5):
        hd.set_nms(ov)
        got = frames_call(hd, frames)
        hd.set_nms(None)
        assert np.array_equal(got, mirror(raw, sizes, ov)), ov
    hd.close()


# ---- 8. DP in groups of whole frames --------------------------------------------------------------------------------------
def test_dp_chunks_of_whole_frames():
    hd = handle(M.synthetic_person_model(thresh=0.0))
    frames = mixed_sizes(1100, [(240, 320), (200, 260), (160, 200), (180, 240)])
    want = frames_call(hd, frames)
    assert len(want) > 0
    hd.set_debug_option(_lib.DP_BUDGET_MB, 1)      # person model: > 1 MB of DP scratch per frame -> one group per frame (4)
    hd.profile(True)
    got = frames_call(hd, frames)
    groups = hd.profile_read()["k_dp_root"][1]       # one root launch per group of frames
    hd.profile(False)
    hd.set_debug_option(_lib.DP_BUDGET_MB, 0)
    assert groups == 4, groups
    assert np.array_equal(got, want)
    hd.profile(True)
    frames_call(hd, frames)
    assert hd.profile_read()["k_dp_root"][1] == 1    # within the default budget: the whole call in one pass
    hd.profile(False)
    assert np.array_equal(frames_call(hd, frames), want)
    hd.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_keep_the_previous_result():
    hd = handle(M.synthetic_tiny_model(thresh=0.4), max_batch=4)
    frames = mixed_sizes(1200, SMALL_MIX)
    want = frames_call(hd, frames)
    p0 = hd.plan(160, 200)
    r0, c0 = int(p0["feat_rows"][0]), int(p0["feat_cols"][0])
    keep = hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0)

    def still_readable():
        assert hd.get_stage(_lib.STAGE_ROOTV, 0, 0, r0, c0).tobytes() == keep.tobytes()

    def call(fr, nframes=None, stride=None):
        fr = [hwc(f) for f in fr]
        d = [(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0] if stride is None else stride) for f in fr]
        arr = _lib.frame_array(d) if d else (_lib.CFrame * 1)()
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        n = C.c_int()
        return hd.lib.pbd_detect_frames(hd.h, len(fr) if nframes is None else nframes, arr, 3, 0, buf.ctypes.data,
                                        hd.max_candidates, C.byref(n))

    assert call(frames, nframes=0) == -1
    still_readable()
    assert call(frames + frames[:1]) == -1                      # 5 > max_batch 4
    still_readable()
    rc = call([frames[0], synth.synthetic_frame(1, 12, 12, 3)])
    assert rc == -1 and "frame 1" in hd.lib.pbd_last_error(hd.h).decode()
    still_readable()
    assert call([frames[0], frames[1]], stride=10) == -1 and "frame 0" in hd.lib.pbd_last_error(hd.h).decode()
    still_readable()
    # a batch in flight
    hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 1, _lib.ptr_array([frames[0]]), 160, 200, 3, 600))
    assert call(frames) == -5
    out = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch_wait(hd.h, out.ctypes.data, hd.max_candidates, C.byref(n)))
    # pbd_dp_argmin after a mixed call
    assert np.array_equal(frames_call(hd, frames), want)
    sc = np.ones(_lib.MAX_LEVELS, np.float32)
    assert hd.lib.pbd_dp_argmin(hd.h, _lib.ptr(sc, C.c_float), out.ctypes.data, 16, C.byref(n)) == -5
    still_readable()
    # device frames whose pointer or pitch is not a multiple of the element size
    import torch
    d = torch.zeros(160 * 200 * 3 + 1, dtype=torch.float32, device="cuda")
    for ptr_off, pitch in ((2, 200 * 12), (0, 200 * 12 + 2)):
        arr = _lib.frame_array([(d.data_ptr() + ptr_off, 100, 120, pitch)])
        rc = hd.lib.pbd_detect_frames_device(hd.h, 1, arr, 3, 5, out.ctypes.data, hd.max_candidates, C.byref(n))
        assert rc == -1 and "frame 0" in hd.lib.pbd_last_error(hd.h).decode()
        still_readable()
    hd.close()


def test_level_sharding_refused_in_either_order():
    frames = mixed_sizes(1300, SMALL_MIX)
    # level sharding set first, on a handle that has made no mixed call
    hd = handle(M.synthetic_tiny_model(thresh=0.4), max_batch=4)
    hd.set_level_shard(0, 2)
    with pytest.raises(PbdError) as e:
        frames_call(hd, frames)
    assert e.value.code == -2
    hd.set_level_shard(0, 1)
    want = frames_call(hd, frames)
    hd.close()
    # a mixed call first: sharding may then be set (it drops the resident result, as for every call), the next mixed call is refused
    hd = handle(M.synthetic_tiny_model(thresh=0.4), max_batch=4)
    assert np.array_equal(frames_call(hd, frames), want)
    hd.set_level_shard(0, 2)
    with pytest.raises(PbdError) as e:
        frames_call(hd, frames)
    assert e.value.code == -2
    hd.set_level_shard(0, 1)
    assert np.array_equal(frames_call(hd, frames), want)
    hd.close()


def test_detect_frames_takes_one_dtype():
    det = detector.PartsBasedDetector(max_batch=4, max_candidates=CAP)
    det.distributeModel(M.synthetic_tiny_model(thresh=0.4))
    frames = mixed_sizes(1400, SMALL_MIX[:2])
    with pytest.raises(PbdError, match="one image dtype"):
        det.detect_batch([frames[0], frames[1].astype(np.float32)])
    with pytest.raises(PbdError):
        det.detect_batch([frames[0].astype(np.int32), frames[1].astype(np.int32)])


# ---- 10. the multi-GPU step's gather of mixed frames (nccl, world size 1, fresh child process) ---------------------------
_CHILD = r'''
import json, os, sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
import torch.distributed as dist
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = "{port}"
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from partsbaseddetector_amd import dist as pd, synth, detector, _lib
from partsbaseddetector_amd import model as M
det = detector.PartsBasedDetector(device=0, max_batch=4, max_candidates=1 << 16)
det.distributeModel(M.synthetic_tiny_model(thresh=0.9))
st = det.hd.stride
batches = [[synth.synthetic_frame(13 * b + i + 1, r, c, 3) for i, (r, c) in enumerate([(120, 150), (96, 128), (140, 111)])]
           for b in range(2)]
def norm(rec, off):
    return [(int(r[0]) - off, int(r[1]), int(r[2]), int(r[3]), int(r[4]), float(r[5:6].view(np.float32)[0]),
             r[8:8 + 4 * int(r[6])].astype(np.int32).tobytes()) for r in rec]
want = [[(c.frame, c.component, c.level, c.root[0], c.root[1], c.score(), c.parts.tobytes()) for c in det.detect_frames(fr)]
        for fr in batches]
dev = [[torch.from_numpy(f).cuda() for f in fr] for fr in batches]
torch.cuda.synchronize()
g = pd.CandidateGatherer(st, cap=1 << 12, device="cuda:0", force_collective=True, cap_full=det.hd.max_candidates)
dg = pd.DeviceBatchGather(det, g)
outs = []
for b in range(2):
    prev = dg.submit_frames([(d.data_ptr(), d.shape[0], d.shape[1], d.stride(0)) for d in dev[b]], 3, frame_offset=10 * b,
                            root_only=True)
    if b > 0:
        outs.append(prev)
outs.append(dg.collect(root_only=True))
res = {{"ok": all(norm(o, 10 * b) == w for b, (o, w) in enumerate(zip(outs, want))), "counts": [len(w) for w in want]}}
det.hd.close()
dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_device_gather_of_mixed_frames(tmp_path):
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
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    assert res["ok"] and min(res["counts"]) > 0, res
