"""The scale-depth pruning rule on the CPU: the numpy yardstick (partsbaseddetector_amd/depthprune.py) against a literal
restatement of include/pbd.h written here, against the decisions stated by hand in tests/depth_prune_cases.py, and the
conditions the GPU tests rely on (every branch reached, every rule matters).  Nothing here needs a GPU.
"""
import ctypes as C
import math

import numpy as np
import pytest

from partsbaseddetector_amd import depthprune, detector
from partsbaseddetector_amd.detector import PbdError

import depth_prune_cases as K


def literal(rect, depth, fx, width, tol, lt=False, holes_are_samples=False, unclipped_points=False, clipped_w=False, all_in_band=False):
    """plausible(rect, depth, fx, width, tol) step by step in Python floats (IEEE doubles) -> (keep, branch); each keyword is one
    changed rule"""
    x, y, w, h = (int(v) for v in rect)
    rows, cols = depth.shape
    if w <= 0:
        return True, "w_nonpositive"
    x1, y1 = (x if x > 0 else 0), (y if y > 0 else 0)
    x2, y2 = (x + w if x + w < cols else cols), (y + h if y + h < rows else rows)
    if x2 - x1 <= 0 or y2 - y1 <= 0:
        return True, "empty_clip"
    fx, width, tol = float(np.float32(fx)), float(np.float32(width)), float(np.float32(tol))
    Z = (fx * width) / float(x2 - x1 if clipped_w else w)
    nvalid = nband = 0
    for j in (0, 1, 2):
        for i in (0, 1, 2):
            if unclipped_points:
                px, py = x + ((2 * i + 1) * w) // 6, y + ((2 * j + 1) * h) // 6
                if not (0 <= px < cols and 0 <= py < rows):
                    continue
            else:
                px, py = x1 + ((2 * i + 1) * (x2 - x1)) // 6, y1 + ((2 * j + 1) * (y2 - y1)) // 6
            d = float(depth[py][px])
            if not holes_are_samples and not (d > 0.0 and d < math.inf):
                continue
            nvalid += 1
            off = math.fabs(d - Z)
            if (off < tol * Z) if lt else (off <= tol * Z):
                nband += 1
    if nvalid == 0:
        return True, "no_valid"
    keep = nband == nvalid if all_in_band else nband > 0
    return keep, "in_band" if keep else "none_in_band"


ALL = [c for dt in K.DTYPES for c in K.build(dt)]


def case_cfg(c):
    return K.cfg(c.image.dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=lambda d: np.dtype(d).name)
def test_yardstick_literal_and_stated_decisions_agree(dtype):
    cases = K.build(dtype)
    assert len(cases) >= 60
    for c in cases:
        keep, branch = literal(c.rect, c.image, *case_cfg(c))
        assert keep == c.keep and branch == c.branch, c.name
        assert depthprune.plausible(c.rect, c.image, *case_cfg(c)) is c.keep, c.name


def test_sample_points():
    assert depthprune.sample_points(K.RECT, K.ROWS, K.COLS) == [(py, px) for py in (11, 17, 23) for px in (16, 24, 32)]
    assert depthprune.sample_points((-10, 8, 24, 18), K.ROWS, K.COLS)[:3] == [(11, 2), (11, 7), (11, 11)]
    assert depthprune.sample_points((K.COLS, 8, 24, 18), K.ROWS, K.COLS) == []
    for cw, want in ((1, [0, 0, 0]), (2, [0, 1, 1]), (3, [0, 1, 2]), (4, [0, 2, 3]), (5, [0, 2, 4]), (6, [1, 3, 5]), (7, [1, 3, 5])):
        got = [px - (K.COLS - cw) for _, px in depthprune.sample_points((K.COLS - cw, 8, 24, 18), K.ROWS, K.COLS)[:3]]
        assert got == want, cw
    for c in ALL:
        if c.branch not in ("w_nonpositive", "empty_clip"):
            assert depthprune.sample_points(c.rect, *c.image.shape) == K.points(c.rect, *c.image.shape), c.name


@pytest.mark.parametrize("max_parts", [3, 26])
@pytest.mark.parametrize("dtype", K.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_case_set_reaches_every_branch_and_cuts_for_real(dtype, max_parts):
    """a condition, not a tolerance: strictly more than none and fewer than all records are kept, every branch is taken"""
    cases = K.build(dtype)
    rec = K.records(cases, max_parts, frame_offset=7)
    depths = [c.image for c in cases]
    kept = depthprune.filter_records(rec, depths, *K.cfg(dtype), frame_offset=7)
    want = rec[[c.keep for c in cases]]
    assert np.array_equal(kept, want) and 0 < len(kept) < len(rec)
    count = {b: sum(c.branch == b for c in cases) for b in K.BRANCHES}
    assert all(n > 0 for n in count.values()), count
    assert count["in_band"] >= 9 * 2 and sum(not c.keep for c in cases) >= 10
    # without the offset every frame index but the first few is another case's image, or out of range
    assert not np.array_equal(depthprune.filter_records(rec, depths, *K.cfg(dtype)), want)


@pytest.mark.parametrize("mutation", ["lt", "holes_are_samples", "unclipped_points", "clipped_w", "all_in_band"])
def test_every_rule_matters(mutation):
    """each single changed rule changes the decision of at least one case, for every depth dtype"""
    for dt in K.DTYPES:
        changed = [c.name for c in K.build(dt) if literal(c.rect, c.image, *case_cfg(c), **{mutation: True})[0] != c.keep]
        assert changed, (mutation, np.dtype(dt).name)


def test_edges_are_the_issue_s():
    """tol = 0.25 and fx * width / w = 1024: 768 and 1280 are kept, 767 and 1281 dropped; in floats one ulp either side"""
    fx, width, tol = K.cfg(np.uint16)
    assert fx * width / K.RECT[2] == 1024 and tol == 0.25
    for dt in (np.uint16, np.float32, np.float64):
        for d, keep in ((768, True), (1280, True), (767, False), (1281, False)):
            assert depthprune.plausible(K.RECT, K.image(dt, d), fx, width, tol) is keep
    for dt in (np.float32, np.float64):
        lo, hi = dt(768), dt(1280)
        for d, keep in ((np.nextafter(lo, dt(0)), False), (np.nextafter(lo, hi), True), (np.nextafter(hi, lo), True),
                        (np.nextafter(hi, dt(np.inf)), False)):
            assert depthprune.plausible(K.RECT, K.image(dt, d), fx, width, tol) is keep


def test_bad_records_are_dropped_and_good_ones_keep_their_bytes():
    for max_parts in (3, 26):
        cases = K.build(np.float32)[:6]
        good = K.records(cases, max_parts, frame_offset=2)
        bad = K.bad_records(max_parts, len(cases), frame_offset=2)
        rec = np.concatenate([bad[:2], good, bad[2:]])
        kept = depthprune.filter_records(rec, [c.image for c in cases], *K.cfg(np.float32), frame_offset=2)
        assert np.array_equal(kept, good[[c.keep for c in cases]]) and 0 < len(kept) < len(good)
    assert depthprune.filter_records(np.zeros((0, 20), np.int32), [], 1, 1, 0).shape == (0, 20)


def test_eligible_planes():
    cases = K.build(np.uint16)[:8]
    rec = K.records(cases, 3)
    rec[:, 0] = 0                                   # one frame: the first case's image for every record
    rec[:, 1], rec[:, 2] = 0, np.arange(8) % 2
    rec[:, 3], rec[:, 4] = np.arange(8), 1
    depth = cases[0].image
    keep = [depthprune.plausible(r[8:12], depth, *K.cfg(np.uint16)) for r in rec]
    planes = depthprune.eligible_planes(rec, [depth], *K.cfg(np.uint16), shapes={(0, 0): (3, 9), (0, 1): (2, 9)})
    assert set(planes) == {(0, 0, 0), (0, 1, 0)} and planes[(0, 0, 0)].shape == (3, 9) and planes[(0, 1, 0)].dtype == np.uint8
    for r, k in zip(rec, keep):
        assert planes[(0, int(r[2]), 0)][1, int(r[3])] == int(k)
    assert sum(int(p.sum()) for p in planes.values()) == sum(keep)


@pytest.fixture(scope="module")
def lib():
    from partsbaseddetector_amd import _lib
    return _lib.load()


def test_symbols_kernel_name_and_null_handle_refusals(lib):
    from partsbaseddetector_amd import _lib
    names = ["pbd_set_depth_prune", "pbd_bind_depth", "pbd_bind_depth_device", "pbd_depth_prune", "pbd_depth_prune_device"]
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert _lib.KERNELS[-1] == "k_depth_prune" and lib.pbd_kernel_name(len(_lib.KERNELS) - 1).decode() == "k_depth_prune"
    cfg = _lib.CDepthPruneCfg(500.0, 0.5, 0.3)
    assert C.sizeof(cfg) == 12
    fr = _lib.frame_array([(0, 4, 4, 4)])
    n = C.c_int(5)
    assert lib.pbd_set_depth_prune(None, C.byref(cfg)) == -1 and lib.pbd_set_depth_prune(None, None) == -1
    assert lib.pbd_bind_depth(None, 1, fr, 0) == -1 and lib.pbd_bind_depth_device(None, 0, None, 0) == -1
    assert lib.pbd_depth_prune(None, C.byref(cfg), 1, fr, 0, None, 0, 0, None, 0, C.byref(n)) == -1
    assert lib.pbd_depth_prune_device(None, C.byref(cfg), 1, fr, 0, None, 0, 0, None, 0) == -1


def test_detector_refuses_bad_parameters_before_any_handle():
    det = detector.PartsBasedDetector(device=0)
    for args in ((0.0, 1.0), (-1.0, 1.0), (math.nan, 1.0), (math.inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, math.inf),
                 (1.0, 1.0, -0.1), (1.0, 1.0, math.nan), (1.0, 1.0, math.inf)):
        with pytest.raises(PbdError):
            det.setDepthPrune(*args)
    det.setDepthPrune(525.0, 0.5)           # kept for distributeModel; tol defaults to 0.3
    assert det._dprune == (525.0, 0.5, 0.3)
    det.setDepthPrune(500.0, 0.4, 0.0)      # tol 0 is legal
    det.setDepthPrune(None)
    assert det._dprune is None
