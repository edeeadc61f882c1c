"""Host logic of mixed-size calls (pbd_detect_frames*), no GPU needed: the virtual level table of a list of frame sizes is
every frame's own pyramid, frame-major, with contiguous cell offsets; the exact convolution's tiles over it cover every
position once; the new entry points are exported and declared in include/pbd.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBIN, INTERVAL = 4, 10


@pytest.fixture(scope="module")
def lib():
    from partsbaseddetector_amd import build, _lib
    build.build_hip()
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.pbd_debug_mixed_plan.restype = C.c_int
    lib.pbd_debug_mixed_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.c_int]
    lib.pbd_debug_seg_tiles.restype = C.c_int
    lib.pbd_debug_seg_tiles.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]
    return lib


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def mixed_plan(lib, sizes, sbin=SBIN, interval=INTERVAL):
    rows = np.array([r for r, c in sizes], np.int32)
    cols = np.array([c for r, c in sizes], np.int32)
    cap = 128 * len(sizes)
    out = np.zeros(7 * cap, np.int32)
    n = lib.pbd_debug_mixed_plan(sbin, interval, len(sizes), ip(rows), ip(cols), ip(out), cap)
    if n < 0:
        return n
    assert n <= cap
    return out[:7 * n].reshape(n, 7)


def random_sizes(rng, n, lo=24):
    return [(int(rng.integers(lo, 1081)), int(rng.integers(lo, 1921))) for _ in range(n)]


# (sbin, interval) of the person model, and a finer one under which a 24 x 24 frame still has `interval` levels
@pytest.mark.parametrize("sbin,interval,lo", [(4, 10, 40), (2, 5, 24)])
def test_mixed_plan_is_every_frame_pyramid_frame_major(lib, sbin, interval, lo):
    from oracle import oracle
    rng = np.random.default_rng(11 + sbin)
    cases = [[(1080, 1920), (720, 1280), (480, 640), (480, 640), (480, 640), (240, 320), (240, 320), (157, 201)],
             [(lo, lo)], [(480, 640)]]
    cases += [random_sizes(rng, int(rng.integers(1, 13)), lo) for _ in range(12)]
    for sizes in cases:
        t = mixed_plan(lib, sizes, sbin, interval)
        k = 0
        cell = 0
        for f, (r, c) in enumerate(sizes):
            lr, lc, _ = oracle.pyramid_plan(r, c, sbin, interval)
            for l in range(len(lr)):
                fr, ll, ir, ic, hr, hc, off = (int(v) for v in t[k])
                assert (fr, ll) == (f, l), (sizes, k)
                assert (ir, ic) == (int(lr[l]), int(lc[l]))
                assert (hr, hc) == tuple(int(v) for v in oracle.hog_dims(int(lr[l]), int(lc[l]), sbin))
                assert off == cell                       # contiguous, non-overlapping, frame-major
                cell += hr * hc
                k += 1
        assert k == len(t)


def test_mixed_plan_refuses_a_frame_too_small(lib):
    assert mixed_plan(lib, [(480, 640), (12, 12)]) == -1
    assert mixed_plan(lib, [(10, 400)]) == -1


def test_seg_tiles_cover_the_virtual_frame_once(lib):
    rng = np.random.default_rng(5)
    for sizes in [[(480, 640), (157, 201), (240, 320)]] + [random_sizes(rng, int(rng.integers(1, 5))) for _ in range(3)]:
        t = mixed_plan(lib, [(max(min(r, 400), 40), max(min(c, 500), 40)) for r, c in sizes])
        rows = np.ascontiguousarray(t[:, 4])
        cols = np.ascontiguousarray(t[:, 5])
        cap = 400000
        buf = np.zeros(16 * cap, np.int32)
        n = lib.pbd_debug_seg_tiles(len(t), ip(rows), ip(cols), 1, ip(buf), cap)
        assert 0 < n <= cap
        cover = [np.zeros((int(h), int(w)), np.int32) for h, w in zip(rows, cols)]
        for rec in buf[:16 * n].reshape(n, 16):
            ns = int(rec[0])
            for s in range(ns):
                f, l, st, x0 = (int(v) for v in rec[4 + 4 * s: 8 + 4 * s])
                assert f == 0
                cover[l][4 * st: 4 * st + 4, x0: x0 + int(rec[1 + s])] += 1
        assert all((c == 1).all() for c in cover)


def test_new_symbols_are_exported(lib):
    from partsbaseddetector_amd import _lib
    for name in ("pbd_detect_frames", "pbd_detect_frames_device", "pbd_detect_frames_device_out", "pbd_debug_mixed_plan"):
        assert hasattr(lib, name), name
    for name in ("pbd_detect_frames", "pbd_detect_frames_device", "pbd_detect_frames_device_out"):
        assert name in _lib.SYMBOLS


def test_header_declares_the_mixed_calls(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check include/pbd.h with")
    src = tmp_path / "use.c"
    src.write_text("""
#include "pbd.h"
int use(pbd_handle *h, const void *a, void *d_payload) {
    pbd_frame fr[2] = {{a, 480, 640, 640 * 3}, {a, 240, 320, 640 * 3}};
    int32_t cand[64]; int n = 0;
    int rc = pbd_detect_frames(h, 2, fr, 3, 0, cand, 1, &n);
    rc |= pbd_detect_frames_device(h, 2, fr, 3, 0, cand, 1, &n);
    rc |= pbd_detect_frames_device_out(h, 2, fr, 3, 0, 5, (int32_t *)d_payload, 1);
    return rc + (int)sizeof(fr[0].stride_bytes);
}
""")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "use.o")])
