"""The Python binding's marshalling rules over a recording stand-in for the library (no GPU, no libpbd_hip.so): what reaches
each pbd_* function and what comes back of what it wrote.

The stand-in records (name, arguments) of every call, returns PBD_OK and stores the count the test chose through every
byref(c_int) argument.  The handle is made without pbd_create and holds just what the methods under test read."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib
from partsbaseddetector_amd.detector import Handle, PbdError, kept_subsequence
from partsbaseddetector_amd.model import synthetic_tiny_model

STRIDE, MAX_PARTS = 20, 3                        # synthetic_tiny_model: three parts, 8 + 4 * 3 words per record


class Recorder:
    def __init__(self):
        self.calls, self.count = [], 0

    def __getattr__(self, name):
        def fn(*args):
            for a in args:
                if isinstance(getattr(a, "_obj", None), C.c_int):
                    a._obj.value = self.count
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def hd():
    h = Handle.__new__(Handle)
    h.lib, h.h, h.stride, h.max_parts, h.dtype = Recorder(), C.c_void_p(1), STRIDE, MAX_PARTS, np.float32
    h.flat = synthetic_tiny_model().flatten()
    yield h
    h.h = None                                   # nothing to destroy


def records(n):
    return np.arange(n * STRIDE, dtype=np.int32).reshape(n, STRIDE)


def frame_fields(arr):
    return [(f.data, f.rows, f.cols, f.stride_bytes) for f in arr]


# ---- the five list-in / list-out calls ------------------------------------------------------------------------------------
DEPTHS = [np.zeros((6, 8), np.uint16), np.zeros((6, 8), np.uint16)]
# name -> (call(hd, records, **kw), pbd function, check of the arguments that precede the records)
LIST_CALLS = {
    "top_k": (lambda h, r, **kw: h.top_k(2, 5, r, **kw), "pbd_top_k", lambda a: a == (2, 5)),
    "depth_consistency": (lambda h, r, **kw: h.depth_consistency(DEPTHS, r, 0.25, **kw), "pbd_depth_consistency",
                          lambda a: (a[0], frame_fields(a[1]), a[2:]) == (2, [(d.ctypes.data, 6, 8, 16) for d in DEPTHS], (2, 0.25))),
    "depth_prune": (lambda h, r, **kw: h.depth_prune(DEPTHS, r, 500.0, 0.5, 0.25, **kw), "pbd_depth_prune",
                    lambda a: ((a[0]._obj.fx, a[0]._obj.width, a[0]._obj.tol), a[1], frame_fields(a[2]), a[3])
                    == ((500.0, 0.5, 0.25), 2, [(d.ctypes.data, 6, 8, 16) for d in DEPTHS], 2)),
    "suppress": (lambda h, r, **kw: h.suppress([(6, 8), (12, 16)], 0.5, r, **kw), "pbd_suppress",
                 lambda a: (a[0], a[1][:2], a[2][:2], a[3]) == (2, [6, 12], [8, 16], 0.5)),
    "part_nms": (lambda h, r, **kw: h.part_nms(2, 0.25, r, 7, **kw), "pbd_part_nms", lambda a: a == (2, 0.25, 7)),
}


@pytest.mark.parametrize("name", sorted(LIST_CALLS))
def test_list_call_arguments(hd, name):
    call, fn, head_ok = LIST_CALLS[name]
    rec = records(3)
    for kw, cap, offset in (({}, 3, 0), ({"capacity": 5}, 5, 0), ({"capacity": 2, "frame_offset": 4}, 2, 4)):
        hd.lib.calls.clear()
        call(hd, rec, **kw)
        (got, args), = hd.lib.calls
        assert got == fn and args[0] is hd.h
        assert head_ok(args[1:-6])
        p_rec, n, off, p_out, capacity, p_n = args[-6:]
        assert (p_rec, n, off, capacity) == (rec.ctypes.data, 3, offset, cap)       # contiguous int32 records go in place
        assert isinstance(p_out, int) and p_out and isinstance(p_n._obj, C.c_int)   # the count comes back by reference
    hd.lib.calls.clear()
    assert call(hd, np.zeros((0, STRIDE), np.int32)).shape == (0, STRIDE)
    args = hd.lib.calls[0][1]
    assert args[-6:-3] == (None, 0, 0) and args[-2] == 0 and args[-3]               # no records: a null pointer, room for none


@pytest.mark.parametrize("name", sorted(LIST_CALLS))
@pytest.mark.parametrize("cap, n, rows", [(4, 2, 2), (4, 4, 4), (4, 6, 4), (None, 3, 3), (0, 0, 0), (0, 2, 0)])
def test_list_call_returns_min_of_count_and_capacity(hd, name, cap, n, rows):
    hd.lib.count = n
    out = LIST_CALLS[name][0](hd, records(3), capacity=cap)
    assert out.shape == (rows, STRIDE) and out.dtype == np.int32 and out.flags.owndata


# ---- image shapes -------------------------------------------------------------------------------------------------------
def test_shape_arrays():
    ir, ic, pr, pc = _lib.shape_arrays([(480, 640), (np.int64(7), 9.0)])
    assert ir.dtype == np.int32 and ic.dtype == np.int32
    assert ir.tolist() == [480, 7] and ic.tolist() == [640, 9]
    assert isinstance(pr, C.POINTER(C.c_int)) and pr[:2] == [480, 7] and pc[:2] == [640, 9]
    assert C.addressof(pr.contents) == ir.ctypes.data and C.addressof(pc.contents) == ic.ctypes.data
    assert [len(a) for a in _lib.shape_arrays([])[:2]] == [0, 0]


# ---- colour frames ------------------------------------------------------------------------------------------------------
def test_image_frames_in_place_or_one_copy():
    wide = np.arange(12 * 20 * 3, dtype=np.uint8).reshape(12, 20, 3)
    hwc, hw, rowview, pixview = np.ascontiguousarray(wide[:, :8]), np.zeros((5, 7), np.float32), wide[:, 3:11], wide[:, ::2]
    for frames, cn, code in (([hwc, rowview, pixview], 3, 0), ([hw], 1, 5)):
        kept, descs, got_cn, got_code = _lib.image_frames(frames)
        assert (got_cn, got_code, len(kept), len(descs)) == (cn, code, len(frames), len(frames))
    kept, descs, _, _ = _lib.image_frames([hwc, rowview, pixview])
    assert frame_fields(descs)[0] == (hwc.ctypes.data, 12, 8, 24)
    assert frame_fields(descs)[1] == (wide.ctypes.data + 9, 12, 8, 60)             # the view's first pixel, the wide image's pitch
    assert frame_fields(descs)[2] == (kept[2].ctypes.data, 12, 10, 30)             # a dense copy
    assert np.shares_memory(kept[0], hwc) and np.shares_memory(kept[1], wide) and not np.shares_memory(kept[2], wide)
    assert np.array_equal(kept[2], pixview) and kept[2].flags.c_contiguous
    (k,), d, _, _ = _lib.image_frames([hw])
    assert frame_fields(d) == [(hw.ctypes.data, 5, 7, 28)] and np.shares_memory(k, hw) and k.shape == (5, 7, 1)
    plane = np.zeros((6, 16), np.uint16)
    (k,), d, cn, code = _lib.image_frames([plane[:, 2:10]])                        # a region of a one-channel image
    assert frame_fields(d) == [(plane.ctypes.data + 4, 6, 8, 32)] and (cn, code) == (1, 2) and np.shares_memory(k, plane)
    flipped = hwc[::-1]                                                            # a negative pitch cannot cross the ABI
    (k,), d, _, _ = _lib.image_frames([flipped])
    assert frame_fields(d) == [(k.ctypes.data, 12, 8, 24)] and not np.shares_memory(k, hwc) and np.array_equal(k, flipped)
    kept, descs, cn, code = _lib.image_frames([])
    assert (kept, len(descs), cn, code) == ([], 0, 3, 0)


def test_image_frames_refusals():
    a = np.zeros((4, 6, 3), np.uint8)
    for bad in ([a, a.astype(np.float32)], [a, a[:, :, :1]], [a, a[:, :, 0]], [a.astype(np.int8)]):
        with pytest.raises(PbdError) as e:
            _lib.image_frames(bad)
        assert e.value.code == -1
    with pytest.raises(PbdError, match="one image dtype") as e:
        _lib.image_frames([a, a.astype(np.float32)], bad_dtype=-2)                 # mixing is the caller's mistake: still -1
    assert e.value.code == -1
    with pytest.raises(PbdError, match="int8") as e:
        _lib.image_frames([a.astype(np.int8)], bad_dtype=-2)                       # the reference's CV_StsUnsupportedFormat
    assert e.value.code == -2


def test_detect_latent_reads_row_strided_crops_in_place(hd):
    wide = np.zeros((12, 20, 3), np.uint8)
    crops = [wide[2:10, 3:11], np.zeros((8, 8, 3), np.uint8)]
    rec, found = hd.detect_latent(crops, np.zeros((2, MAX_PARTS, 4), np.int32), 0.5)
    (name, args), = hd.lib.calls
    assert name == "pbd_detect_latent" and args[1] == 2 and args[3:5] == (3, 0) and args[6] is None and args[7] == 0.5
    assert frame_fields(args[2]) == [(wide.ctypes.data + 2 * 60 + 9, 8, 8, 60), (crops[1].ctypes.data, 8, 8, 24)]
    assert rec.shape == (2, STRIDE) and found.shape == (2,)


# ---- depth images -------------------------------------------------------------------------------------------------------
def test_depth_frames():
    wide = np.arange(6 * 16, dtype=np.uint16).reshape(6, 16)
    dense, rowview, pixview = np.ascontiguousarray(wide[:, :8]), wide[:, 3:11], wide[:, ::2]
    kept, descs, code = _lib.depth_frames([dense, rowview, pixview])
    assert code == 2 and frame_fields(descs) == [(dense.ctypes.data, 6, 8, 16), (wide.ctypes.data + 6, 6, 8, 32),
                                                 (kept[2].ctypes.data, 6, 8, 16)]
    assert np.shares_memory(kept[0], dense) and np.shares_memory(kept[1], wide) and not np.shares_memory(kept[2], wide)
    assert np.array_equal(kept[2], pixview)
    assert _lib.depth_frames([np.zeros((2, 3), np.float64)])[2] == 6
    for bad in ([dense, dense.astype(np.float32)], [dense.astype(np.int16)]):
        with pytest.raises(PbdError, match="one depth dtype per call: uint8, uint16, float32 or float64") as e:
            _lib.depth_frames(bad)
        assert e.value.code == -1


@pytest.mark.parametrize("call, fn, at", [
    (lambda h, d: h.boxes3d(d, [(6, 8)] * 2, records(2)), "pbd_boxes3d", 1),
    (lambda h, d: h.boxes3d_camera(d, [(6, 8)] * 2, [type("K", (), dict(fx=1, fy=1, cx=0, cy=0, tx=0, ty=0))] * 2, records(2)),
     "pbd_boxes3d_camera", 1),
    (lambda h, d: h.depth_consistency(d, records(2)), "pbd_depth_consistency", 1),
    (lambda h, d: h.depth_prune(d, records(2), 500.0, 0.5, 0.3), "pbd_depth_prune", 2),
    (lambda h, d: h.bind_depth(d), "pbd_bind_depth", 1)])
def test_every_depth_entry_point_uses_the_one_rule(hd, call, fn, at):
    wide = np.zeros((6, 16), np.float32)
    call(hd, [wide[:, 3:11], np.zeros((6, 8), np.float32)])
    (name, args), = hd.lib.calls
    assert name == fn and args[at] == 2 and args[at + 2] == 5
    assert frame_fields(args[at + 1])[0] == (wide.ctypes.data + 12, 6, 8, 64)      # in place, the wide image's pitch
    with pytest.raises(PbdError, match="one depth dtype per call: uint8, uint16, float32 or float64"):
        call(hd, [wide, wide.astype(np.float64)])


# ---- packed planes and segments -----------------------------------------------------------------------------------------
def test_pack_arrays_and_split():
    a, b, c = np.arange(6, dtype=np.float32).reshape(2, 3), np.arange(20, dtype=np.float32).reshape(4, 5)[:, ::2], np.zeros((0, 7), np.float32)
    arrs, real, src, msk = _lib.pack_arrays([a, b, c], None, "t")
    assert real == _lib.REAL_F32 and msk is None and src.dtype == np.float32
    assert src.tolist() == a.ravel().tolist() + b.ravel().tolist() and [x.shape for x in arrs] == [(2, 3), (4, 3), (0, 7)]
    bools = [np.array([[1, 0, 1], [0, 0, 1]], bool), np.ones((4, 3), bool), np.zeros((0, 7), bool)]
    bytes_ = [np.array([[7, 0, 255], [0, 0, 2]], np.uint8), np.full((4, 3), 9, np.uint8), np.zeros((0, 7), np.uint8)]
    m1, m2 = _lib.pack_arrays([a, b, c], bools, "t")[3], _lib.pack_arrays([a, b, c], bytes_, "t")[3]
    assert m1.dtype == np.uint8 and m1.tolist() == [1, 0, 1, 0, 0, 1] + [1] * 12 and np.array_equal(m1, m2)
    out = _lib.split_arrays(np.arange(18, dtype=np.uint8), arrs)
    assert [o.shape for o in out] == [(2, 3), (4, 3), (0, 7)] and out[0].ravel().tolist() == list(range(6)) and out[1][0].tolist() == [6, 7, 8]
    assert _lib.pack_arrays([a.astype(np.float64)], None, "t")[1] == _lib.REAL_F64
    arrs, real, src, msk = _lib.pack_arrays([], [], "t")
    assert (arrs, real, src.size, msk.size) == ([], _lib.REAL_F32, 0, 0) and _lib.split_arrays(np.zeros(0, np.uint8), []) == []
    for bad, masks in (([a.astype(np.float16)], None), ([a, a.astype(np.float64)], None), ([a], [np.ones((3, 2), bool)]), ([a, b], [bools[0]])):
        with pytest.raises(PbdError, match="^PBD_ERR_INVALID: t: ") as e:
            _lib.pack_arrays(bad, masks, "t")
        assert e.value.code == -1


def test_grid_nms_and_top_k_cells_calls(hd):
    planes = [np.ones((2, 3), np.float32), np.ones((4, 5), np.float32), np.zeros((0, 7), np.float32)]
    out = hd.grid_nms(planes, 2, [np.ones(p.shape, bool) for p in planes])
    (name, a), = hd.lib.calls
    assert name == "pbd_grid_nms" and (a[1], a[2][:3], a[3][:3], a[4], a[7]) == (3, [2, 4, 0], [3, 5, 7], _lib.REAL_F32, 2) and a[5] and a[6] and a[8]
    assert [o.shape for o in out] == [p.shape for p in planes] and all(o.dtype == np.uint8 for o in out)
    hd.lib.calls.clear()
    out = hd.top_k_cells([p.astype(np.float64) for p in planes], 4)
    (name, a), = hd.lib.calls
    assert name == "pbd_top_k_cells" and (a[1], a[2][:3], a[3], a[5], a[6]) == (3, [6, 20, 0], _lib.REAL_F64, None, 4) and a[4] and a[7]
    assert [o.shape for o in out] == [p.shape for p in planes]
    with pytest.raises(PbdError, match="2-D"):
        hd.grid_nms([np.ones(5, np.float32)], 2)


# ---- small rules --------------------------------------------------------------------------------------------------------
def test_opt_ptr_and_real_code():
    a = np.zeros((2, 3), np.int32)
    assert _lib.opt_ptr(a) == a.ctypes.data and _lib.opt_ptr(a[:0]) is None and _lib.opt_ptr(np.zeros((0, 4))) is None
    assert (_lib.real_code(np.float32), _lib.real_code("float64"), _lib.real_code(np.dtype(np.float64))) == (0, 1, 1)
    for bad in (np.float16, np.int32):
        with pytest.raises(PbdError) as e:
            _lib.real_code(bad)
        assert e.value.code == -1


def test_host_list_cached_buffer_is_reused(hd):
    hd.max_candidates, hd.lib.count = 4, 0
    buf, n = hd.wait_batch(raw=True)
    assert (n, buf.size) == (0, 4 * STRIDE) and hd.lib.calls[-1][0] == "pbd_detect_batch_wait" and hd.lib.calls[-1][1][1:3] == (buf.ctypes.data, 4)
    assert hd.detect_batch_device(0x1000, 2, 6, 8, 3, capacity=3, raw=True)[0] is buf                 # one buffer for both, not reallocated
    assert hd.lib.calls[-1] == ("pbd_detect_batch_device", hd.lib.calls[-1][1]) and hd.lib.calls[-1][1][1:6] == (2, 0x1000, 6, 8, 3)
    assert hd.wait_batch(capacity=0, raw=True)[0] is buf and hd.lib.calls[-1][1][2] == 4              # 0: the default capacity
    big = hd.wait_batch(capacity=9, raw=True)[0]
    assert big is not buf and big.size == 9 * STRIDE and hd.wait_batch(raw=True)[0] is big             # grown once, kept
    assert hd.wait_batch() == []
    fresh = [hd.detect(np.zeros((6, 8, 3), np.uint8)), hd.detect_frames(_lib.frame_array([]), 3, 0)]
    assert fresh == [[], []] and hd._buf is big
    hd.dp_argmin([1.0], capacity=0)
    assert hd.lib.calls[-1][0] == "pbd_dp_argmin" and hd.lib.calls[-1][1][3] == 0                      # here 0 is a capacity


# ---- the kept records are the input's, in order -------------------------------------------------------------------------
def test_kept_subsequence():
    rec = records(5)
    rec[2] = rec[1]                                                                # two equal adjacent records
    items = list("abcde")
    assert kept_subsequence(items, rec, rec) == items
    assert kept_subsequence(items, rec, rec[:0]) == []
    assert kept_subsequence(items, rec, rec[[0, 2, 4]]) == ["a", "b", "e"]         # one of the equal pair kept: the earlier item
    assert kept_subsequence(items, rec, rec[[1, 2, 3]]) == ["b", "c", "d"]         # both kept
    assert kept_subsequence(items, records(5), records(5)[::2]) == ["a", "c", "e"]          # every second record
    assert kept_subsequence(items, records(5), records(5)[1::2]) == ["b", "d"]
    assert kept_subsequence([], rec[:0], rec[:0]) == []
