"""The grid NMS yardstick (gridnms.grid_nms_ref) against a literal restatement of src/nms.cpp:84-129, hand-worked answers, the
contract's consequences and mutations of its rules -- no GPU.  The last test checks, on the CPU oracle's rootv, that the inputs of
tests/test_gpu_root_nms.py make the root NMS do real work."""
import numpy as np
import pytest

from partsbaseddetector_amd import gridnms
from partsbaseddetector_amd import model as M

import grid_nms_cases as G
from grid_nms_cases import ROOT_NMS_SIZES, ROOT_NMS_THRESH, root_nms_frames

CASES = G.cases()
SMALL = [c for c in CASES if not c.big]
DTYPES = (np.float32, np.float64)


# ---- the second formulation: nms.cpp's own Range / blockmask arithmetic, statement by statement -----------------------------
def min_max_loc(sub, msk):
    """cv::minMaxLoc(sub, NULL, &vmax, NULL, &ijmax, msk): the largest element under a non-zero mask byte and the first
    place it occurs in raster order, as (value, (x, y)); None where nothing is under the mask (the project's decision)"""
    best, loc = None, None
    for i in range(sub.shape[0]):
        for j in range(sub.shape[1]):
            if msk[i, j] and (best is None or sub[i, j] > best):
                best, loc = sub[i, j], (j, i)
    return None if loc is None else (best, loc)


def literal(src, sz, mask=None, ge=False, last=False, keep_own_block=False, empty_is_zero=False):
    """nonMaximaSuppression(src, sz, dst, mask); NaN elements are masked out first.  The keyword arguments are the mutations.
    Returns dst and the events of G's docstring."""
    M_, N_ = src.shape
    elig = (~np.isnan(src)).astype(np.uint8) * 255
    if mask is not None:
        elig = elig * (np.asarray(mask) != 0)
    block = 255 * np.ones((2 * sz + 1, 2 * sz + 1), np.uint8)
    dst = np.zeros(src.shape, np.uint8)
    ev = set()
    for m in range(0, M_, sz + 1):
        for n in range(0, N_, sz + 1):
            ic = (m, min(m + sz + 1, M_))
            jc = (n, min(n + sz + 1, N_))
            if ic[1] - ic[0] < sz + 1 or jc[1] - jc[0] < sz + 1:
                ev.add("clipped_block")
            sub, smask = src[ic[0]:ic[1], jc[0]:jc[1]], elig[ic[0]:ic[1], jc[0]:jc[1]]
            got = min_max_loc(sub[::-1, ::-1], smask[::-1, ::-1]) if last else min_max_loc(sub, smask)
            if got is None:
                ev.add("empty_block")
                continue
            vcmax, ijmax = got
            if last:
                ijmax = (sub.shape[1] - 1 - ijmax[0], sub.shape[0] - 1 - ijmax[1])
            if np.count_nonzero((sub == vcmax) & (smask != 0)) > 1:
                ev.add("tie_in_block")
            cc = (ijmax[0] + jc[0], ijmax[1] + ic[0])           # Point(x, y)
            in_ = (max(cc[1] - sz, 0), min(cc[1] + sz + 1, M_))
            jn = (max(cc[0] - sz, 0), min(cc[0] + sz + 1, N_))
            if in_[1] - in_[0] < 2 * sz + 1 or jn[1] - jn[0] < 2 * sz + 1:
                ev.add("clipped_window")
            blockmask = block[0:in_[1] - in_[0], 0:jn[1] - jn[0]].copy()
            iis = (ic[0] - in_[0], min(ic[0] - in_[0] + sz + 1, in_[1] - in_[0]))
            jis = (jc[0] - jn[0], min(jc[0] - jn[0] + sz + 1, jn[1] - jn[0]))
            if not keep_own_block:
                blockmask[iis[0]:iis[1], jis[0]:jis[1]] = 0
            win = src[in_[0]:in_[1], jn[0]:jn[1]]
            nmask = (elig[in_[0]:in_[1], jn[0]:jn[1]] != 0) * blockmask
            got = min_max_loc(win, nmask)
            if got is None:
                ev.add("empty_neighbourhood")
                keep = vcmax > 0 if empty_is_zero else True
            else:
                vnmax = got[0]
                keep = vcmax >= vnmax if ge else vcmax > vnmax
                if vcmax == vnmax:
                    ev.add("tie_across")
                elif vcmax < vnmax:
                    ev.add("beaten")
                    # beaten only from the four diagonally adjacent blocks
                    yy, xx = np.nonzero((nmask != 0) & (win >= vcmax))
                    if all((y + in_[0] < ic[0] or y + in_[0] >= ic[1]) and (x + jn[0] < jc[0] or x + jn[0] >= jc[1]) for y, x in zip(yy, xx)):
                        ev.add("diagonal_only")
            if keep:
                dst[cc[1], cc[0]] = 255
                ev.add("kept")
                with np.errstate(invalid="ignore"):
                    if np.any((blockmask != 0) & (nmask == 0) & (win > vcmax)):
                        ev.add("masked_larger")
    return dst, ev


def maxima(dst):
    return [(int(y), int(x)) for y, x in zip(*np.nonzero(dst))]


# ---- tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_two_formulations_agree(case, dtype):
    src = case.plane(dtype)
    got = gridnms.grid_nms_ref(src, case.sz, case.mask)
    assert got.dtype == np.uint8 and got.shape == src.shape and set(np.unique(got)) <= {0, 255}
    want, _ = literal(src, case.sz, case.mask)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_hand_worked_answers(dtype):
    n = 0
    for case in CASES:
        want = case.answer(dtype)
        if want is None:
            continue
        assert maxima(gridnms.grid_nms_ref(case.plane(dtype), case.sz, case.mask)) == sorted(want), case.name
        n += 1
    assert n >= 24


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_maxima_are_more_than_sz_apart_and_one_per_block(case):
    src = case.plane(np.float64)
    dst = gridnms.grid_nms_ref(src, case.sz, case.mask)
    pts = np.array(maxima(dst)).reshape(-1, 2)
    bs = case.sz + 1
    assert len({(y // bs, x // bs) for y, x in pts}) == len(pts)
    if len(pts) > 1:
        d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
        d[np.arange(len(pts)), np.arange(len(pts))] = case.sz + 1
        assert d.min() > case.sz
    ok = gridnms.eligible(src, case.mask)
    assert not np.any((dst != 0) & ~ok)
    if case.sz == 0:
        assert np.array_equal(dst != 0, ok)               # blocks of 1 x 1: every eligible element is kept


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_each_case_reaches_what_it_promises(case):
    _, ev = literal(case.plane(np.float32 if case.big else np.float64), case.sz, case.mask)
    assert set(case.reach) <= ev, (case.name, set(case.reach) - ev)


def test_the_cases_cover_the_issue_list():
    names = {c.name for c in CASES}
    for sz in G.SIZES:
        assert f"quantised_sz{sz}" in names and f"holes_sz{sz}" in names
    from partsbaseddetector_amd import _lib
    assert _lib.GRID_NMS_WAVE_SZ - 1 in G.SIZES and _lib.GRID_NMS_WAVE_SZ in G.SIZES     # both sides of the variant switch
    ev = set()
    for c in SMALL:
        ev |= literal(c.plane(np.float64), c.sz, c.mask)[1]
    assert ev >= {"clipped_block", "clipped_window", "empty_block", "empty_neighbourhood", "tie_in_block", "tie_across",
                  "diagonal_only", "masked_larger", "beaten", "kept"}
    planes = G.many_planes()
    assert len(planes) >= 3000 and any(p.size == 0 for p in planes)
    assert sum(-(-p.shape[0] // 2) * -(-p.shape[1] // 2) for p in planes) > 2048 * 4     # more blocks than a capped grid has waves


@pytest.mark.parametrize("mutation", ["ge", "last", "keep_own_block", "empty_is_zero"])
def test_every_rule_matters(mutation):
    """each mutation of the contract changes the result of some small case"""
    changed = [c.name for c in SMALL
               if not np.array_equal(literal(c.plane(np.float64), c.sz, c.mask, **{mutation: True})[0],
                                     gridnms.grid_nms_ref(c.plane(np.float64), c.sz, c.mask))]
    assert changed, mutation


def test_ref_refuses_bad_arguments():
    with pytest.raises(ValueError):
        gridnms.grid_nms_ref(np.zeros((2, 2)), -1)
    with pytest.raises(ValueError):
        gridnms.grid_nms_ref(np.zeros(4), 1)
    with pytest.raises(ValueError):
        gridnms.grid_nms_ref(np.zeros((2, 2)), 32768)


# ---- the detect path's inputs (tests/test_gpu_root_nms.py) on the CPU oracle ---------------------------------------------------
def oracle_root_planes(oracle, flat, im):
    """{(level, component): rootv plane} of one frame"""
    feats, _ = oracle.features_pyramid(flat, im)
    out = {}
    for l, f in enumerate(feats):
        if f.size == 0:
            continue
        resp = oracle.responses(flat, f)
        for c in range(flat.ncomponents):
            out[(l, c)] = oracle.dp_min(flat, c, resp)[3]
    return out


def test_detect_path_inputs_make_the_step_do_real_work(oracle):
    model = M.synthetic_tiny_model(thresh=ROOT_NMS_THRESH)
    flat = model.flatten()
    planes = oracle_root_planes(oracle, flat, root_nms_frames()[0])
    thr = np.float32(flat.thresh)
    found = sum(int(np.count_nonzero(p > thr)) for p in planes.values())
    assert found >= 50
    for sz in ROOT_NMS_SIZES:
        kept = dropped_best = 0
        kept_worst = np.inf
        for p in planes.values():
            hit = p > thr
            keep = gridnms.grid_nms_ref(p, sz, hit) != 0
            kept += int(keep.sum())
            if keep.any():
                kept_worst = min(kept_worst, float(p[keep].min()))
            if (hit & ~keep).any():
                dropped_best = max(dropped_best, float(p[hit & ~keep].max()))
        assert 1 <= kept <= found // 2, (sz, kept, found)
        assert dropped_best > kept_worst, (sz, dropped_best, kept_worst)      # not a top-k: a dropped root outscores a kept one
