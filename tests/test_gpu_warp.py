"""Warped positives on the device (pbd_warp_positives*): every comparison is byte equality (tobytes()) against the numpy
yardstick partsbaseddetector_amd/warp.py (the CPU oracle's resize and HOG on a clamped gather), for T = float and double.

Frames are synthetic, 80 x 96 and 90 x 120 pixels (rows x cols).  The standard box list covers windows inside the frame,
crossing each edge, wholly outside, 1 x 1, an exact copy, a strong shrink, a strong aspect change, two boxes on one frame, frames
named out of order and a frame with no box."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth, warp
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
LOW = -1e9
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def one_part_model(k, sbin=4, seed=5):
    return M.synthetic_model(seed=seed, pa=[0], nmix=1, ksize=k, sbin=sbin, interval=5, thresh=LOW, name=f"one_part_k{k}_s{sbin}")


def handle(model, dtype=np.float32, max_batch=4):
    return detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18, max_batch=max_batch)


_FRAMES = {}


def frames_u8(cn=3):
    """three frames: 80 x 96, 90 x 120 (no box names it in the standard list), 80 x 96"""
    if cn not in _FRAMES:
        fr = [synth.synthetic_frame(71, 80, 96), synth.synthetic_frame(72, 90, 120), synth.synthetic_frame(73, 80, 96, kind="noise")]
        _FRAMES[cn] = [np.ascontiguousarray(f[:, :, :cn]) for f in fr]
    return _FRAMES[cn]


def frames_of(dtype, cn=3):
    fr = frames_u8(cn)
    if dtype == np.uint8:
        return fr
    if dtype == np.uint16:
        return [(f.astype(np.uint16) * 257) ^ (f.astype(np.uint16)[::-1, ::-1] * 3) for f in fr]   # the full 16-bit range
    return [(f.astype(dtype) / dtype(255) - dtype(0.25)) * dtype(3) for f in fr]                 # negative values too


def standard_boxes(k, sbin):
    """(frame, x1, y1, x2, y2): frames 2 and 0 (80 x 96) out of order, frame 1 without a box"""
    R, Cc = 80, 96
    side = k * sbin
    cx, cy = min(30, Cc - side - 2 * sbin), min(25, R - side - 2 * sbin)
    return np.array([
        (2, 20, 15, 59, 49),                       # inside
        (0, -5, 20, 30, 50),                       # crosses the left edge
        (0, Cc - 30, 20, Cc + 6, 55),              # right
        (2, 30, -8, 70, 30),                       # top
        (2, 30, R - 25, 70, R + 5),                # bottom
        (0, -4, -6, 40, 30),                       # top and left
        (0, -70, -60, -30, -25),                   # wholly outside
        (2, Cc + 20, R + 10, Cc + 60, R + 50),     # wholly outside, the other corner
        (0, 40, 40, 40, 40),                       # 1 x 1
        (0, max(cx, 0), max(cy, 0), max(cx, 0) + side - 1, max(cy, 0) + side - 1),   # the window is the patch: an exact copy
        (2, 8, 0, 87, 79),                         # 80 px wide: a strong shrink
        (0, 20, 40, 79, 49),                       # 60 x 10: a strong aspect change
        (2, -1, -1, 1, 1),                         # a half at or below zero with k = 6
    ], np.int32)


def same(got, ref):
    for g, r, name in zip(got, ref, ("hdr", "values", "kept")):
        assert g.shape == r.shape and g.dtype == r.dtype, name
        assert g.tobytes() == r.tobytes(), name


def run_case(model, frames, boxes, dtype, filter=0, bias=0, skip_small=False):
    flat = model.flatten()
    ref = warp.warp_examples(flat, frames, boxes, filter, bias, skip_small, dtype)
    if skip_small:     # stated on the yardstick before the GPU is asked
        assert ref[2].sum() >= len(boxes) // 2 and ref[2].min() == 0
    hd = handle(model, dtype)
    try:
        got = hd.warp_positives(frames, boxes, filter, bias, skip_small)
        same(got, ref)
    finally:
        hd.close()
    return ref


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sbin", [4, 8])
@pytest.mark.parametrize("k", [1, 3, 5, 6])
def test_shapes_bgr8(k, sbin, dtype):
    hdr, vals, kept = run_case(one_part_model(k, sbin), frames_u8(), standard_boxes(k, sbin), dtype)
    assert kept.all() and (hdr[:, 3] == 1 + k * k * 32).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sbin3(dtype):
    run_case(one_part_model(5, 3), frames_u8(), standard_boxes(5, 3), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pix", [np.uint8, np.float64])
def test_large_patch_k12_sbin8(pix, dtype):
    """P = 112: a 64F three-channel patch is 301 KB, no whole-patch LDS plan fits"""
    run_case(one_part_model(12, 8), frames_of(pix), standard_boxes(12, 8)[[0, 1, 6, 8, 10, 11]], dtype)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pix,cn", [(np.uint8, 1), (np.uint16, 3), (np.uint16, 1), (np.float32, 3), (np.float64, 3), (np.float64, 1)])
def test_depths_and_channels(pix, cn, dtype):
    run_case(one_part_model(5, 4), frames_of(pix, cn), standard_boxes(5, 4), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_sizes_and_skip_rule(dtype):
    """boxes on frames of both sizes in one call; the skip rule at area == minsize (kept) and minsize - 1 (skipped)"""
    k, sbin = 5, 4
    side = k * sbin                                  # minsize = 400
    boxes = np.array([(1, 10, 10, 99, 69), (0, 5, 5, 5 + side - 1, 5 + side - 1), (1, 100, 70, 130, 95),
                      (0, 3, 3, 3 + 398, 3),         # 399 x 1: skipped
                      (1, 3, 3, 3 + 399, 3),         # 400 x 1: kept
                      (2, 40, 40, 40, 40),           # 1 x 1: skipped
                      (1, 0, 0, 18, 20), (2, 60, 50, 95, 79)], np.int32)
    hdr, vals, kept = run_case(one_part_model(k, sbin), frames_u8(), boxes, dtype, skip_small=True)
    assert kept.tolist() == [1, 1, 1, 0, 1, 0, 0, 1]
    assert (hdr[kept == 0, 2] == -1).all() and not vals[kept == 0].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_part_handle_filter_and_bias_offsets(dtype):
    """filter / bias of a later part: blocks at that part's offsets in the model vector; bias -1: one block"""
    model = M.synthetic_model(seed=11, pa=[0, 1, 1], nmix=2, ksize=[5, 3], sbin=4, interval=5, thresh=LOW)
    flat = model.flatten()
    _, fbase, _ = E.vector_offsets(flat)
    boxes = standard_boxes(3, 4)[[0, 1, 9, 10]]
    for f, b in ((3, 4), (4, -1), (0, 0)):
        k = int(flat.filter_ksize[f])
        hdr, vals, kept = run_case(model, frames_u8(), boxes, dtype, filter=f, bias=b)
        n = k * k * 32
        want = ([b, 1] if b >= 0 else []) + [fbase + int(flat.filter_offset[f]), n]
        assert (hdr[:, 2] == len(want) // 2).all() and (hdr[:, 3] == n + (b >= 0)).all()
        assert (hdr[:, 4:4 + len(want)] == want).all()


# ---- the device form ------------------------------------------------------------------------------------------------------
def device_call(hd, descs, cn, depth_code, boxes, filter, bias, skip_small, id_offset, capacity, dtype):
    import torch
    hw, vw = hd.example_stride()
    pay = torch.full((1 + capacity * hd.stride,), -3, dtype=torch.int32, device="cuda")
    dh = torch.zeros(capacity * hw, dtype=torch.int32, device="cuda")
    dv = torch.zeros(capacity * vw, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    hd.warp_positives_device(descs, cn, depth_code, boxes, filter, bias, skip_small, id_offset, pay.data_ptr(), capacity,
                             dh.data_ptr(), dv.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return pay, dh, dv


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pix", [np.uint8, np.float32])
def test_device_form_on_regions_of_a_larger_image(pix, dtype):
    """frames are regions of larger device images, read through the pitch: the clamp stops at the region, not at the parent"""
    import torch
    k, sbin = 5, 4
    model = one_part_model(k, sbin)
    flat = model.flatten()
    rng = np.random.default_rng(9)
    parents = [rng.integers(0, 256, (130, 170, 3)).astype(pix), rng.integers(0, 256, (120, 150, 3)).astype(pix)]
    if pix != np.uint8:
        parents = [p / pix(7) for p in parents]
    rects = [(10, 20, 80, 96), (0, 0, 90, 120), (40, 54, 80, 96)]      # y0, x0, rows, cols; the last ends at its parent's corner
    owner = [0, 1, 1]
    regions = [np.ascontiguousarray(parents[o][y:y + r, x:x + c]) for o, (y, x, r, c) in zip(owner, rects)]
    dev = [torch.from_numpy(p).cuda() for p in parents]
    es = np.dtype(pix).itemsize
    descs = [(dev[o].data_ptr() + (y * parents[o].shape[1] + x) * 3 * es, r, c, parents[o].shape[1] * 3 * es)
             for o, (y, x, r, c) in zip(owner, rects)]
    boxes = np.concatenate([standard_boxes(k, sbin), [(1, 100, 70, 130, 95), (1, -3, -3, 30, 30), (2, 60, 50, 95, 79), (2, 90, 75, 97, 81)]])
    boxes = boxes.astype(np.int32)
    for skip in (False, True):
        ref = warp.warp_examples(flat, regions, boxes, 0, 0, skip, dtype)
        if skip:
            assert ref[2].sum() >= len(boxes) // 2 and ref[2].min() == 0
        hd = handle(model, dtype)
        try:
            host = hd.warp_positives(regions, boxes, 0, 0, skip)
            same(host, ref)
            cap, id_offset = len(boxes) + 3, 40
            pay, dh, dv = device_call(hd, descs, 3, _lib.DEPTH_CODE[np.dtype(pix)], boxes, 0, 0, skip, id_offset, cap, dtype)
            n = len(boxes)
            hw, vw = hd.example_stride()
            assert dh.cpu().numpy()[:n * hw].tobytes() == ref[0].tobytes()
            assert dv.cpu().numpy()[:n * vw].tobytes() == ref[1].tobytes()
            assert not dh.cpu().numpy()[n * hw:].any() and not dv.cpu().numpy()[n * vw:].any()
            p = pay.cpu().numpy()
            assert p[0] == n
            rec = p[1:1 + n * hd.stride].reshape(n, hd.stride)
            want = np.zeros_like(rec)
            want[:, 0] = id_offset + np.arange(n)
            assert np.array_equal(rec, want)
            assert (p[1 + n * hd.stride:] == -3).all()                 # nothing past the records
            with pytest.raises(PbdError) as e:                         # nboxes > capacity
                device_call(hd, descs, 3, _lib.DEPTH_CODE[np.dtype(pix)], boxes, 0, 0, skip, 0, n - 1, dtype)
            assert e.value.code == -4
            pay0, _, _ = device_call(hd, descs, 3, _lib.DEPTH_CODE[np.dtype(pix)], boxes[:0], 0, 0, skip, 0, 4, dtype)
            assert int(pay0[0].item()) == 0
        finally:
            hd.close()


# ---- the QP ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_qp_entries_host_device_and_yardstick(dtype):
    import torch
    k, sbin = 5, 4
    model = one_part_model(k, sbin)
    flat = model.flatten()
    frames = frames_u8()
    boxes = np.concatenate([standard_boxes(k, sbin), [(1, 10, 10, 99, 69), (1, 3, 3, 10, 10)]]).astype(np.int32)
    ref = warp.warp_examples(flat, frames, boxes, 0, 0, True, dtype)
    assert ref[2].sum() >= len(boxes) // 2 and ref[2].min() == 0
    n, id_base, id_offset = len(boxes), 1000, 17
    ids = np.zeros((n, 5), np.int32)
    ids[:, 0] = 1
    ids[:, 1] = id_base + id_offset + np.arange(n)
    hd = handle(model, dtype)
    try:
        hdr, vals, kept = hd.warp_positives(frames, boxes, 0, 0, True)
        same((hdr, vals, kept), ref)
        qh, qd, qr = Q.QP(hd, 64), Q.QP(hd, 64), Q.QPRef(flat, 64)
        assert qh.add(hd, hdr, vals, ids=ids) == kept.sum()
        dev = [torch.from_numpy(f).cuda() for f in frames]
        descs = [(t.data_ptr(), f.shape[0], f.shape[1], f.strides[0]) for t, f in zip(dev, frames)]
        pay, dh, dv = device_call(hd, descs, 3, 0, boxes, 0, 0, True, id_offset, n, dtype)
        taken = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        qd.add_device(hd, pay.data_ptr(), n, dh.data_ptr(), dv.data_ptr(), 1, id_base, taken.data_ptr())
        assert int(taken.item()) == kept.sum()
        assert qr.add(ref[0], ref[1], ids) == kept.sum()
        a, b, r = qh.entries(), qd.entries(), qr.entries()
        for u, v, w in zip(a, b, r):
            assert u.tobytes() == v.tobytes() and u.tobytes() == np.ascontiguousarray(w).tobytes()
        assert np.array_equal(b[4], ids[kept == 1])
    finally:
        hd.close()


# ---- score identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_score_identity(k, dtype):
    """w . x of a kept box = the root filter's response at the centre cell of the patch's feature map (pbd_conv_pdf on the
    same features) + the bias, within examples.rounding_bound"""
    model = one_part_model(k, 4)
    flat = model.flatten()
    boxes = standard_boxes(k, 4)[[0, 1, 6, 10, 11]]
    hd = handle(model, dtype)
    try:
        hdr, vals, kept = hd.warp_positives(frames_u8(), boxes, 0, 0, False)
        assert kept.all()
        w = hd.model_vector()
        n = k * k * 32
        feats = [np.ascontiguousarray(v[1:1 + n]).reshape(k, k * 32) for v in vals]
        resp = detector.SpatialConvolutionEngine(hd).pdf(feats)
        got = E.dot(hdr, vals, w)
        bound = E.rounding_bound(flat, hdr, vals, w, dtype)
        for i in range(len(boxes)):
            want = float(resp[i][0][k // 2, k // 2]) + float(flat.biasw[0])
            assert abs(got[i] - want) <= bound[i], (i, got[i], want, bound[i])
    finally:
        hd.close()


# ---- the detect path and the resident result ------------------------------------------------------------------------------
def records(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], _lib.DEPTH_CODE[fr[0].dtype], buf.ctypes.data,
                                      hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_detect_path_untouched_and_resident_result_dropped(dtype):
    import torch
    model = M.synthetic_tiny_model(thresh=LOW)
    flat = model.flatten()
    frames = frames_u8()
    boxes = standard_boxes(5, 4)
    ref = warp.warp_examples(flat, frames, boxes, 0, 0, False, dtype)
    hd = handle(model, dtype)
    try:
        before = records(hd, frames[:2])
        assert len(before) > 0
        ex_before = hd.examples(before[:4])
        same(hd.warp_positives(frames, boxes, 0, 0, False), ref)
        # the warp worked in the pyramid and HOG workspaces: no resident result until the next detect call
        with pytest.raises(PbdError) as e:
            hd.examples(before[:4])
        assert e.value.code == -5
        pay = torch.zeros(1 + 8 * hd.stride, dtype=torch.int32, device="cuda")
        assert hd.lib.pbd_argmin_device_out(hd.h, 0, pay.data_ptr(), 8) == -5
        with pytest.raises(PbdError):
            hd.get_stage(_lib.STAGE_FEATURES, 0, 0, 4, 4)
        after = records(hd, frames[:2])
        assert after.tobytes() == before.tobytes()
        ex_after = hd.examples(after[:4])
        assert ex_after[0].tobytes() == ex_before[0].tobytes() and ex_after[1].tobytes() == ex_before[1].tobytes()
        # a call without boxes and a refused call leave the resident result
        assert len(hd.warp_positives(frames, boxes[:0], 0, 0, False)[0]) == 0
        with pytest.raises(PbdError):
            hd.warp_positives(frames, boxes, 99, 0, False)
        assert hd.examples(after[:4])[1].tobytes() == ex_before[1].tobytes()
    finally:
        hd.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def raw(hd, descs, nframes, cn, depth, boxes, filter=0, bias=0, null=None):
    """pbd_warp_positives with explicit arguments; the status code"""
    hw, vw = hd.example_stride()
    n = len(boxes)
    hdr, vals, kept = np.zeros((max(n, 1), hw), np.int32), np.zeros((max(n, 1), vw), hd.dtype), np.zeros(max(n, 1), np.int32)
    bx = np.ascontiguousarray(boxes, np.int32)
    args = {"frames": descs, "boxes": bx.ctypes.data if n else None, "hdr": hdr.ctypes.data, "values": vals.ctypes.data, "kept": kept.ctypes.data}
    if null:
        args[null] = None
    return hd.lib.pbd_warp_positives(hd.h, nframes, args["frames"], cn, depth, n, args["boxes"], filter, bias, 0, args["hdr"],
                                     args["values"], args["kept"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(dtype):
    model = M.synthetic_tiny_model(thresh=2.0)
    flat = model.flatten()
    frames = frames_u8()
    boxes = standard_boxes(5, 4)[[0, 1, 6, 9]]
    ref = warp.warp_examples(flat, frames, boxes, 1, 2, False, dtype)
    hd = handle(model, dtype)
    msg = lambda: hd.lib.pbd_last_error(hd.h).decode()
    try:
        def valid():
            same(hd.warp_positives(frames, boxes, 1, 2, False), ref)

        def descs_of(fr, pitch=None):
            return _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0] if pitch is None else pitch) for f in fr])

        valid()
        d = descs_of(frames)
        nb, nf = len(flat.biasw), flat.nfilters
        for kw in ({"filter": -1}, {"filter": nf}, {"bias": -2}, {"bias": nb}):
            assert raw(hd, d, 3, 3, 0, boxes, **kw) == -1, kw
            assert str(list(kw.values())[0]) in msg()
            valid()
        bad = boxes.copy(); bad[2, 0] = 3
        assert raw(hd, d, 3, 3, 0, bad) == -1 and "box 2" in msg()
        bad = boxes.copy(); bad[1, 0] = -1
        assert raw(hd, d, 3, 3, 0, bad) == -1 and "box 1" in msg()
        bad = boxes.copy(); bad[3, 3] = bad[3, 1] - 1
        assert raw(hd, d, 3, 3, 0, bad) == -1 and "box 3" in msg()
        bad = boxes.copy(); bad[0, 4] = bad[0, 2] - 1
        assert raw(hd, d, 3, 3, 0, bad) == -1 and "box 0" in msg()
        valid()
        # the frame refusals of pbd_detect_frames
        assert raw(hd, d, 3, 2, 0, boxes) == -1 and "channels" in msg()
        assert raw(hd, d, 3, 3, 1, boxes) == -2 and "depth" in msg()
        assert raw(hd, descs_of(frames, pitch=96 * 3 - 1), 3, 3, 0, boxes) == -1 and "frame 0" in msg()
        empty = _lib.frame_array([(frames[0].ctypes.data, 80, 96, 288), (frames[1].ctypes.data, 0, 120, 360), (frames[2].ctypes.data, 80, 96, 288)])
        assert raw(hd, empty, 3, 3, 0, boxes) == -1 and "frame 1" in msg()
        valid()
        f32 = frames_of(np.float32)
        f32 = [f.copy() for f in f32]
        f32[2][5, 7, 1] = np.nan
        assert raw(hd, descs_of(f32), 3, 3, 5, boxes) == -1 and "frame 2" in msg() and "NaN" in msg()
        f32[2][5, 7, 1] = np.inf
        assert raw(hd, descs_of(f32), 3, 3, 5, boxes) == -1 and "frame 2" in msg()
        # NULL pointers with boxes
        for name in ("frames", "boxes", "hdr", "values", "kept"):
            assert raw(hd, d, 3, 3, 0, boxes, null=name) == -1, name
        assert raw(hd, d, 3, 3, 0, boxes[:0]) == 0                      # no boxes: PBD_OK
        valid()
        # while a batch is in flight
        ptrs = _lib.ptr_array([frames[0]])
        hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 1, ptrs, 80, 96, 3, 288))
        assert raw(hd, d, 3, 3, 0, boxes) == -5
        buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
        n = C.c_int()
        hd.check(hd.lib.pbd_detect_batch_wait(hd.h, buf.ctypes.data, hd.max_candidates, C.byref(n)))
        valid()
    finally:
        hd.close()
