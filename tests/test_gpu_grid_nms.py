"""pbd_grid_nms / pbd_grid_nms_device (Handle.grid_nms, PartsBasedDetector.gridNMS) against gridnms.grid_nms_ref, byte for byte,
on every built case of grid_nms_cases.py: float32 and float64 planes, on a float and on a double handle, host and device forms,
both kernel variants (one lane or one wave per block) at every size, a call of 3000 planes and one of more blocks than the capped
grid has threads."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, gridnms
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

import grid_nms_cases as G

pytestmark = pytest.mark.gpu
CASES = G.cases()
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def handles():
    hs = {"float": detector.Handle(M.synthetic_tiny_model(), device=0, max_batch=1),
          "double": detector.Handle(M.synthetic_tiny_model(), device=0, max_batch=1, real_type=_lib.REAL_F64)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def refs():
    """the yardstick's answer for every (case, dtype), computed once"""
    return {(c.name, np.dtype(dt)): gridnms.grid_nms_ref(c.plane(dt), c.sz, c.mask) for c in CASES for dt in DTYPES}


def groups():
    """the cases that can share a call: one window size, all with a mask or all without; empty planes between the others"""
    out = {}
    for c in CASES:
        out.setdefault((c.sz, c.mask is not None), []).append(c)
    return list(out.items())


def check_group(hd, key, cs, dt, refs):
    sz, masked = key
    got = hd.grid_nms([c.plane(dt) for c in cs], sz, [c.mask for c in cs] if masked else None)
    for c, g in zip(cs, got):
        assert np.array_equal(g, refs[(c.name, np.dtype(dt))]), (c.name, np.dtype(dt).name, sz)


@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("which", ["float", "double"])
def test_host_form_equals_the_yardstick(handles, refs, which, dt):
    for key, cs in groups():
        check_group(handles[which], key, cs, dt, refs)


@pytest.mark.parametrize("lanes", [1, 64])
def test_both_kernel_variants_at_every_size(handles, refs, lanes):
    hd = handles["float"]
    hd.set_debug_option(_lib.GRID_NMS_LANES, lanes)
    try:
        for dt in DTYPES:
            for key, cs in groups():
                check_group(hd, key, cs, dt, refs)
    finally:
        hd.set_debug_option(_lib.GRID_NMS_LANES, 0)


@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f64"))
def test_device_form_equals_the_yardstick(handles, refs, dt):
    import torch
    hd = handles["float"]
    for (sz, masked), cs in groups():
        planes = [c.plane(dt) for c in cs]
        src = torch.from_numpy(np.concatenate([p.ravel() for p in planes] + [np.zeros(1, dt)])).cuda()
        msk = torch.from_numpy(np.concatenate([c.mask.ravel() for c in cs])).cuda() if masked else None
        dst = torch.full((src.numel(),), 7, dtype=torch.uint8, device="cuda")
        hd.grid_nms_device([p.shape[0] for p in planes], [p.shape[1] for p in planes], _lib.REAL_F32 if dt == np.float32 else _lib.REAL_F64,
                           src.data_ptr(), msk.data_ptr() if masked and msk.numel() else None, sz, dst.data_ptr())
        hd.check(hd.lib.pbd_synchronize(hd.h))
        got = dst.cpu().numpy()
        assert got[-1] == 7                                   # nothing past the last plane is written
        off = 0
        for c, p in zip(cs, planes):
            assert np.array_equal(got[off:off + p.size].reshape(p.shape), refs[(c.name, np.dtype(dt))]), (c.name, sz)
            off += p.size


def test_one_handle_five_sizes_in_turn(handles, refs):
    hd = handles["double"]
    by_sz = {c.sz: c for c in CASES if c.name.startswith("holes_sz")}
    for sz in (7, 1, 100, 0, 4, 7):
        c = by_sz[sz]
        assert np.array_equal(hd.grid_nms([c.plane(np.float32)], sz)[0], refs[(c.name, np.dtype(np.float32))]), sz


@pytest.mark.parametrize("lanes", [1, 64])
def test_three_thousand_planes_in_one_call(handles, lanes):
    hd = handles["float"]
    planes = [p.astype(np.float32) for p in G.many_planes()]
    want = [gridnms.grid_nms_ref(p, 1) for p in planes]
    hd.set_debug_option(_lib.GRID_NMS_LANES, lanes)
    try:
        got = hd.grid_nms(planes, 1)
    finally:
        hd.set_debug_option(_lib.GRID_NMS_LANES, 0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_more_blocks_than_the_capped_grid_has_threads(handles):
    """sz = 0: blocks of one cell, every eligible element is kept (checked for the yardstick in test_grid_nms_cpu.py); 525 000
    blocks are more than 2048 workgroups of 256 threads"""
    rng = np.random.default_rng(3)
    p = rng.standard_normal((750, 700)).astype(np.float32)
    p[rng.random(p.shape) < 0.01] = np.nan
    assert p.size > 2048 * 256
    got = handles["float"].grid_nms([p], 0)[0]
    assert np.array_equal(got, (~np.isnan(p)).astype(np.uint8) * 255)


def test_detector_method(handles):
    det = detector.PartsBasedDetector(device=0)
    det.distributeModel(M.synthetic_tiny_model())
    c = next(c for c in CASES if c.name == "random_mask")
    assert np.array_equal(det.gridNMS(c.plane(np.float32), c.sz, c.mask), gridnms.grid_nms_ref(c.plane(np.float32), c.sz, c.mask))
    det.hd.close()


def test_refused_arguments(handles):
    hd = handles["float"]
    lib, h = hd.lib, hd.h
    src = np.zeros(12, np.float32)
    dst = np.zeros(12, np.uint8)
    rows, cols = np.array([3], np.int32), np.array([4], np.int32)
    pr, pc = _lib.ptr(rows, C.c_int), _lib.ptr(cols, C.c_int)

    def refused(*args, fn=lib.pbd_grid_nms):
        assert fn(h, *args) == -1, args
        assert lib.pbd_last_error(h).decode(), args
    ok = (1, pr, pc, _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data)
    assert lib.pbd_grid_nms(h, *ok) == 0
    for fn in (lib.pbd_grid_nms, lib.pbd_grid_nms_device):
        refused(1, pr, pc, _lib.REAL_F32, src.ctypes.data, None, -1, dst.ctypes.data, fn=fn)          # sz < 0
        refused(1, pr, pc, _lib.REAL_F32, src.ctypes.data, None, 32768, dst.ctypes.data, fn=fn)       # sz > 32767
        refused(-1, pr, pc, _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)          # nplanes < 0
        refused(1, pr, pc, 2, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)                       # another real_code
        refused(1, pr, pc, _lib.REAL_F32, None, None, 1, dst.ctypes.data, fn=fn)                      # NULL src
        refused(1, pr, pc, _lib.REAL_F32, src.ctypes.data, None, 1, None, fn=fn)                      # NULL dst
        refused(1, None, pc, _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)         # NULL rows
        refused(1, pr, None, _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)         # NULL cols
        neg = np.array([-3], np.int32)
        refused(1, _lib.ptr(neg, C.c_int), pc, _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)
        refused(1, pr, _lib.ptr(neg, C.c_int), _lib.REAL_F32, src.ctypes.data, None, 1, dst.ctypes.data, fn=fn)
        assert fn(h, 0, None, None, _lib.REAL_F32, None, None, 1, None) == 0                          # no planes: nothing to do
    with pytest.raises(PbdError):
        hd.grid_nms([np.zeros((2, 2), np.int32)], 1)
    with pytest.raises(PbdError) as e:
        hd.set_debug_option(_lib.GRID_NMS_LANES, 32)
    assert e.value.code == -1
