"""The top-K yardstick (topk.top_k_cells_ref / top_k_records_ref) against hand-worked answers, a second formulation (repeated
"take the best that is left"), the events the built cases promise, mutations of the rule, the shard property, and the symbols and
refusals that need no GPU.  The last test checks, on the CPU oracle's rootv, that the inputs of tests/test_gpu_top_k.py make the
detect-path selection do real work."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import topk

import top_k_cases as T
from top_k_cases import oracle_frame_values

CASES = T.cases()
SMALL = [c for c in CASES if not c.big]
DTYPES = (np.float32, np.float64)


# ---- the second formulation: K rounds of "the best element that is left", the rule's comparisons spelled out ------------------
def literal(v, k, mask=None, later=False, ge=False, neg_zero_below=False, keep_nan=False, ignore_mask=False):
    """the kept indices of one segment, ascending.  The keyword arguments are the mutations."""
    left = [i for i in range(len(v))
            if (keep_nan or not np.isnan(v[i])) and (ignore_mask or mask is None or mask[i] != 0)]

    def better(a, b):
        va, vb = v[a], v[b]
        if neg_zero_below and va == 0 and vb == 0 and np.signbit(va) != np.signbit(vb):
            return bool(np.signbit(vb))
        if va > vb:
            return True
        if va == vb or (np.isnan(va) and np.isnan(vb)):
            return a > b if later else a < b
        return False
    kept = []
    for _ in range(min(k, len(left))):
        best = left[0]
        for i in left[1:]:
            if better(i, best):
                best = i
        kept.append(best)
        left.remove(best)
    if ge and kept:
        pivot = v[kept[-1]]
        kept += [i for i in left if v[i] >= pivot]
    return sorted(kept)


def kept_indices(dst):
    return [int(i) for i in np.flatnonzero(np.asarray(dst).ravel())]


def key_bits(v):
    """the order-preserving unsigned key of the kernel, for the events only"""
    v = np.where(v == 0, np.zeros_like(v), v)
    u = v.view(np.uint32 if v.dtype == np.float32 else np.uint64)
    top = u.dtype.type(1) << u.dtype.type(u.dtype.itemsize * 8 - 1)
    return np.where(u & top, ~u, u | top)


def events(v, k, mask, kept):
    """the events of top_k_cases' docstring one segment reaches, from its values, its mask and the kept bytes"""
    ev = set()
    n = len(v)
    ok = topk.eligible(v, mask)
    ne = int(ok.sum())
    keep = np.asarray(kept) != 0
    ev.add("empty_segment" if n == 0 else "")
    if n > T.TILE:
        ev.add("multi_tile")
    ev.add("k_zero" if k == 0 else "k_below" if k < ne else "k_at" if k == ne and ne > 0 else "k_above" if k > ne else "")
    if np.isnan(v).any():
        ev.add("nan_hole")
    if mask is not None and n and not np.any(np.asarray(mask) != 0):
        ev.add("mask_all_zero")
    if mask is not None and (~np.isnan(v)).any():
        best = np.nanmax(v)
        if not np.any(ok & (v == best)):
            ev.add("mask_hides_best")
    if ne >= 2 and len(np.unique(v[ok] + 0.0)) == 1:
        ev.add("all_equal")
    if ne >= 2:
        kb = key_bits(v[ok])
        if len(np.unique(kb)) > 1 and (kb.max() ^ kb.min()) < 256:
            ev.add("low_byte_only")
    if keep.any() and (ok & ~keep).any():
        pivot = v[keep].min()
        tk, td = keep & (v == pivot), ok & ~keep & (v == pivot)
        if td.any():
            ev.add("cut_in_tie")
            if tk.sum() >= 2 and td.sum() >= 2:
                ev.add("two_each_side")
            if len({int(i) // T.TILE for i in np.flatnonzero(tk)}) > 1:
                ev.add("tie_across_tiles")
            if pivot == 0 and len({bool(s) for s in np.signbit(v[tk | td])}) == 2:
                ev.add("zeros_cut")
            if np.isposinf(pivot):
                ev.add("inf_tie")
        dropped = v[ok & ~keep]
        if np.any(np.isin(-v[keep][v[keep] != 0], dropped)):
            ev.add("sign_only")
    ev.discard("")
    return ev


def case_events(case, dtype):
    ev = set()
    vals, masks = case.values(dtype), case.mask_list()
    for i, v in enumerate(vals):
        m = None if masks is None else masks[i]
        ev |= events(v, case.k, m, topk.top_k_cells_ref(v, case.k, m))
    if len(vals) > 2048:
        ev.add("longer_than_grid")
    return ev


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_hand_worked_answers(dtype):
    n = 0
    for case in CASES:
        want = case.answer(dtype)
        if want is None:
            continue
        masks = case.mask_list()
        for i, v in enumerate(case.values(dtype)):
            got = topk.top_k_cells_ref(v, case.k, None if masks is None else masks[i])
            assert got.dtype == np.uint8 and got.shape == v.shape and set(np.unique(got)) <= {0, 255}
            assert kept_indices(got) == want[i], (case.name, i)
        n += 1
    assert n >= 25


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_ref_equals_the_second_formulation(case, dtype):
    masks = case.mask_list()
    for i, v in enumerate(case.values(dtype)):
        if len(v) * min(case.k, len(v)) > 3_000_000:
            continue
        m = None if masks is None else masks[i]
        assert kept_indices(topk.top_k_cells_ref(v, case.k, m)) == literal(v, case.k, m), (case.name, i)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kept_count_and_eligibility(case):
    masks = case.mask_list()
    for i, v in enumerate(case.values(np.float64)):
        m = None if masks is None else masks[i]
        dst = topk.top_k_cells_ref(v, case.k, m) != 0
        ok = topk.eligible(v, m)
        assert dst.sum() == min(case.k, ok.sum()) and not np.any(dst & ~ok)
        if dst.any() and (ok & ~dst).any():
            assert v[dst].min() >= v[ok & ~dst].max()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_each_case_reaches_what_it_promises(case):
    ev = case_events(case, np.float64)
    assert set(case.reach) <= ev, (case.name, set(case.reach) - ev)
    if "low_byte_only" in case.reach:
        assert "low_byte_only" in case_events(case, np.float32)


def test_the_cases_cover_the_issue_list():
    ev = set()
    for c in CASES:
        ev |= case_events(c, np.float64)
    assert ev >= set(T.EVENTS), set(T.EVENTS) - ev
    by = {c.name: c for c in CASES}
    assert tuple(len(s) for s in by["lengths_k64"].segs) == (0, 1, 63, 64, 65, 1023, 1024, 1025)
    assert any(len(s) == 70000 for s in by["long_between_short"].segs) and len(by["tiny_3000"].segs) == 3000
    pair = by["f64_difference_below_float"]
    assert pair.answer(np.float32) != pair.answer(np.float64)
    v32 = pair.values(np.float32)[0]
    assert v32[0] == v32[1] and pair.segs[0][1] - pair.segs[0][0] == 2.0 ** -40
    segs = T.many_segments()
    assert len(segs) > 4096 * 4 and any(len(s) == 0 for s in segs)       # more segments than a capped grid has waves
    assert sum(-(-len(s) // T.TILE) for s in by["medium_5000"].segs) > 4096   # more tiles than a capped grid has workgroups
    names = {n for n, *_ in T.RECORD_CASES}
    assert {"frames_without_records", "nan_score", "cut_inside_a_run"} <= names


@pytest.mark.parametrize("mutation", ["later", "ge", "neg_zero_below", "keep_nan", "ignore_mask"])
def test_every_rule_matters(mutation):
    """each mutation of the rule changes the answer of some small case"""
    changed = []
    for c in SMALL:
        masks = c.mask_list()
        for i, v in enumerate(c.values(np.float64)):
            if len(v) > 300:
                continue
            m = None if masks is None else masks[i]
            if literal(v, c.k, m, **{mutation: True}) != kept_indices(topk.top_k_cells_ref(v, c.k, m)):
                changed.append(c.name)
    assert changed, mutation


def test_union_of_shard_top_ks_contains_and_reselects_the_global_top_k():
    """records cut into shards by level: top-K of the union of the shards' top-Ks, put in canonical order, is the global top-K"""
    rng = np.random.default_rng(5)
    for trial in range(20):
        n, k = int(rng.integers(1, 200)), int(rng.integers(0, 40))
        rec = np.zeros((n, 12), np.int32)
        rec[:, 0] = np.sort(rng.integers(0, 3, n))
        rec[:, 2] = rng.integers(0, 6, n)                                         # level
        rec[:, 3], rec[:, 4] = rng.integers(0, 50, n), rng.integers(0, 50, n)     # x, y
        rec[:, 5] = T.stepped(trial, n, 6).astype(np.float32).view(np.int32)     # few distinct scores: ties everywhere
        rec[:, 6] = 1
        rec = np.unique(rec, axis=0)
        rec = topk.canonical_order(rec)
        want = topk.top_k_records_ref(rec, k)
        shards = [topk.top_k_records_ref(rec[rec[:, 2] % 2 == r], k) for r in (0, 1)]
        merged = topk.canonical_order(np.concatenate(shards))
        assert np.array_equal(topk.top_k_records_ref(merged, k), want)
        assert {tuple(r) for r in want} <= {tuple(r) for r in merged}


def test_record_cases_by_hand_and_against_the_cells_form():
    by = {n: (s, k) for n, s, k, _ in T.RECORD_CASES}
    rec = T.record_list(12, *by["cut_inside_a_run"][:1])
    assert np.array_equal(topk.top_k_records_ref(rec, 3), rec[[0, 1, 2]])
    rec = T.record_list(12, by["frames_without_records"][0])
    assert np.array_equal(topk.top_k_records_ref(rec, 2), rec[[0, 1, 2, 3, 5]])
    rec = T.record_list(12, by["nan_score"][0])
    assert np.array_equal(topk.top_k_records_ref(rec, 3), rec[[1, 3]])
    rec = T.record_list(12, by["special"][0])
    assert np.array_equal(topk.top_k_records_ref(rec, 5), rec[sorted(T.SPECIAL_ORDER[:5])])
    assert len(topk.top_k_records_ref(T.record_list(12, by["k_zero"][0]), 0)) == 0
    for name, scores, k, reach in T.RECORD_CASES:
        ev = set()
        for f, s in scores.items():
            v = np.array(s, np.float32)
            ev |= events(v, k, None, topk.top_k_cells_ref(v, k))
        assert set(reach) <= ev, (name, set(reach) - ev)
    rec = T.random_records(12, 5000, 7, 3)
    assert len(rec) == 5000 and np.all(np.diff(rec[:, 0]) >= 0)
    got = topk.top_k_records_ref(rec, 40)
    assert 0 < len(got) <= 7 * 40 and not np.isnan(got[:, 5].copy().view(np.float32)).any()


def test_ref_refuses_a_negative_k():
    with pytest.raises(ValueError):
        topk.top_k_cells_ref(np.zeros(3), -1)


# ---- symbols and refusals that need no GPU ---------------------------------------------------------------------------------
def test_symbols_and_null_handle_refusals():
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = _lib.load()
    for n in ["pbd_top_k_cells", "pbd_top_k_cells_device", "pbd_set_top_k", "pbd_top_k", "pbd_top_k_device"]:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    i = _lib.KERNELS.index("k_top_k")
    assert _lib.KERNELS[i - 1] == "k_grid_nms" and _lib.KERNELS[i + 1] == "k_depth_prune" and i + 2 == len(_lib.KERNELS)
    lib.pbd_kernel_name.restype = C.c_char_p
    assert lib.pbd_kernel_name(i).decode() == "k_top_k" and lib.pbd_kernel_name(i + 1).decode() == "k_depth_prune"
    ln = (C.c_longlong * 1)(4)
    n = C.c_int(5)
    assert lib.pbd_set_top_k(None, 3) == -1
    assert lib.pbd_top_k_cells(None, 1, ln, _lib.REAL_F32, None, None, 1, None) == -1
    assert lib.pbd_top_k_cells_device(None, 0, None, _lib.REAL_F32, None, None, 1, None) == -1
    assert lib.pbd_top_k(None, 1, 1, None, 0, 0, None, 0, C.byref(n)) == -1
    assert lib.pbd_top_k_device(None, 1, 1, None, 0, 0, None, 0) == -1


def test_detector_refuses_bad_parameters_before_any_handle():
    from partsbaseddetector_amd import detector
    from partsbaseddetector_amd.detector import PbdError
    det = detector.PartsBasedDetector.__new__(detector.PartsBasedDetector)
    det.hd, det._top_k = None, 0
    for k in (-1, (1 << 30) + 1):
        with pytest.raises(PbdError):
            det.setTopK(k)
    det.setTopK(1 << 30)
    det.setTopK(5)                          # kept for distributeModel
    assert det._top_k == 5
    det.setTopK(0)
    assert det._top_k == 0


# ---- the detect path's inputs (tests/test_gpu_top_k.py) on the CPU oracle -------------------------------------------------------
def test_detect_path_inputs_make_the_selection_do_real_work(oracle):
    flat = M.synthetic_tiny_model(thresh=T.TOP_K_THRESH).flatten()
    frames = T.top_k_frames()
    thr = np.float32(flat.thresh)
    # a plain frame: well over the largest small K eligible cells, so every K of the sweep but the last one cuts
    v = oracle_frame_values(oracle, flat, frames[0])
    hit = v > thr
    assert hit.sum() > 65 * 4 and len(np.unique(v[hit])) == hit.sum()
    # the tiled frame: its second and third best cells are exactly equal, so the cut of K = 2 falls inside a tie and must take the
    # first of the two in raster order
    v = oracle_frame_values(oracle, flat, frames[1])
    hit = v > thr
    top = np.sort(v[hit])[::-1]
    assert hit.sum() > 65 * 4 and top[0] > top[1] == top[2] > top[3]
    first, second = np.flatnonzero(hit & (v == top[1]))
    assert kept_indices(topk.top_k_cells_ref(v, 2, hit)) == sorted([int(np.flatnonzero(v == top[0])[0]), int(first)]) and first < second
    assert "cut_in_tie" in events(v, 2, hit, topk.top_k_cells_ref(v, 2, hit))
    # the constant frame with the threshold at 0: long runs of equal values, most K cut inside a tie
    v = oracle_frame_values(oracle, flat, frames[3])
    hit = v > np.float32(0)
    vals, counts = np.unique(v[hit], return_counts=True)
    assert hit.sum() > 1000 and len(vals) < hit.sum() // 4 and counts.max() > 500
    for k in (64, 65):                      # both sides of a wave's worth of roots cut inside a run
        assert "cut_in_tie" in events(v, k, hit, topk.top_k_cells_ref(v, k, hit)), k
