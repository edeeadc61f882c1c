"""The scale-NMS yardstick (scalenms.keep_records / keep_planes; include/pbd.h states the rule): hand-worked record lists, the two
formulations against each other on built pyramids and on the CPU oracle's root planes, the rule's properties, mutations of every
clause, the pinned counts of two real frames, the constant frame's cross-level ties, and the symbols and refusals that need no
GPU."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import scalenms as S
from partsbaseddetector_amd import synth

import scale_nms_cases as T

DTYPES = (np.float32, np.float64)


def both_forms(levels, ks, thresh, dl):
    """(records of the eligible cells, their scores, kept mask by all pairs) after checking the plane form -- with and without
    its window bound -- against it"""
    rec, sc = S.plane_records(levels, ks, T.eligible_planes(levels, thresh))
    keep = S.keep_records(rec, dl, sc)
    for use_window in (True, False):
        got, _ = S.plane_records(levels, ks, S.keep_planes(levels, ks, thresh, dl, use_window))
        assert np.array_equal(got, rec[keep]), (dl, use_window)
    return rec, sc, keep


def check_properties(rec, sc, keep, dl):
    """symmetric relation, no two survivors neighbours, the best root survives"""
    n = len(rec)
    for i in range(n):
        for j in range(i + 1, n):
            a = S.neighbours(rec[i, 8:12], rec[i, 2], rec[j, 8:12], rec[j, 2], dl)
            assert a == S.neighbours(rec[j, 8:12], rec[j, 2], rec[i, 8:12], rec[i, 2], dl)
            assert not (a and keep[i] and keep[j] and rec[i, 0] == rec[j, 0]), (i, j)
    ok = ~np.isnan(sc)
    if ok.any():
        best = np.flatnonzero(ok & (sc == np.nanmax(sc)))[0]       # the earliest of the largest
        assert keep[best]


# ---- record lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.RECORD_CASES, ids=[c[0] for c in T.RECORD_CASES])
def test_record_cases_by_hand(case):
    name, rows, dl, want = case
    rec = T.record_list(rows)
    keep = S.keep_records(rec, dl)
    assert list(np.flatnonzero(keep)) == want
    assert np.array_equal(keep, T.keep_mutant(rec, dl))
    assert np.array_equal(S.filter_records(rec, dl), rec[want])
    check_properties(rec, np.ascontiguousarray(rec[:, 5]).view(np.float32), keep, dl)
    # the same list in frame 7 of a call whose frames start at 7
    assert np.array_equal(S.keep_records(T.record_list(rows, frame_offset=7), dl, frame_offset=7, nframes=5), keep)


def test_bad_frames_and_part_counts_are_dropped_and_beat_nobody():
    rows = [(0, 3, 0, 1.0, 0, 0, 10, 10), (0, 3, 0, 5.0, 0, 0, 10, 10), (0, 3, 0, 6.0, 0, 0, 10, 10), (9, 3, 0, 7.0, 0, 0, 10, 10)]
    rec = T.record_list(rows)
    rec[1, 6] = 0                       # no parts
    rec[2, 6] = 2                       # more parts than a stride of 12 holds
    assert list(np.flatnonzero(S.keep_records(rec, 0, nframes=2))) == [0]
    assert list(np.flatnonzero(S.keep_records(rec, 0))) == [0, 3]
    with pytest.raises(ValueError):
        S.keep_records(rec, 256)
    with pytest.raises(ValueError):
        S.keep_records(rec, -1)


def test_random_lists_against_the_plain_loops_and_properties():
    for seed, n, nframes in ((1, 0, 1), (2, 1, 1), (3, 150, 3), (4, 300, 2)):
        rec = T.random_records(n, nframes, seed)
        for dl in (0, 1, 3, 255):
            keep = S.keep_records(rec, dl)
            assert np.array_equal(keep, T.keep_mutant(rec, dl)), (seed, dl)
            if n:
                check_properties(rec, np.ascontiguousarray(rec[:, 5]).view(np.float32), keep, dl)


def test_dl_above_the_level_count_means_all_levels():
    rec = T.random_records(200, 1, 9, nlevels=8)
    assert np.array_equal(S.keep_records(rec, 7), S.keep_records(rec, 255))
    assert not np.array_equal(S.keep_records(rec, 6), S.keep_records(rec, 255))


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_every_mutation_changes_a_result(mutation):
    changed = [name for name, rows, dl, want in T.RECORD_CASES
               if list(np.flatnonzero(T.keep_mutant(T.record_list(rows), dl, mutation))) != want]
    assert changed, mutation


# ---- built pyramids: the two formulations -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_plane_form_equals_all_pairs_on_built_pyramids(dtype):
    for name, levels, ks, thresh in T.plane_frames(dtype):
        for dl in (0, 1, 2, 255):
            rec, sc, keep = both_forms(levels, ks, thresh, dl)
            assert 0 < keep.sum() < len(rec), (name, dl)
            if len(rec) < 400:
                check_properties(rec, sc, keep, dl)


def test_built_pyramids_reach_what_they_promise():
    frames = {n: (lv, ks, th) for n, lv, ks, th in T.plane_frames(np.float32)}
    lv, ks, th = frames["padded_2_2"]
    rec, _ = S.plane_records(lv, ks, T.eligible_planes(lv, th))
    assert (rec[:, 8] < 0).any() and (rec[:, 3] < 2).any()              # roots on the pad, rectangles left of the frame
    lv, ks, th = frames["filter_sides_and_components"]
    rec, _ = S.plane_records(lv, ks, T.eligible_planes(lv, th))
    assert len(np.unique(rec[:, 1])) == 3
    assert len({(r[2], r[10]) for r in rec if r[2] == 0}) >= 5          # several widths on one level
    lv, ks, th = frames["fine_octave_and_empty_level"]
    assert all(a.scale < b.scale for a, b in zip(lv, lv[1:])) and lv[-1].rootv[0].size == 0
    lv, ks, th = frames["every_cell_eligible"]
    assert sum(int(e.sum()) for row in T.eligible_planes(lv, th) for e in row) == sum(v.size for L in lv for v in L.rootv)


def test_window_contains_every_neighbour_of_random_rectangles():
    rng = np.random.default_rng(8)
    for _ in range(300):
        s = np.float32(rng.choice([0.7, 1.0, 2.0, 3.3, 4.0, 7.9, 16.0]))
        pad, n, kmax = int(rng.integers(0, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 9))
        xa, wa = int(rng.integers(-40, 200)), int(rng.integers(0, 60))
        wmax = S.round_mul(kmax, s, np.float32) + 1
        c0, c1 = S.window(xa, wa, wmax, float(s), pad, n)
        assert 0 <= c0 and c1 <= n
        for c in list(range(0, c0)) + list(range(max(c1, 0), n)):
            for ks in range(1, kmax + 1):
                xb, _, wb, _ = S.part_rect(c, 0, ks, s, np.float32, pad, 0)
                assert wb <= wmax
                assert not (wa > 0 and 2 * xa <= 2 * xb + wb < 2 * (xa + wa)), (xa, wa, s, pad, c, ks)
                assert not (wb > 0 and 2 * xb <= 2 * xa + wa < 2 * (xb + wb)), (xa, wa, s, pad, c, ks)


# ---- real frames on the CPU oracle --------------------------------------------------------------------------------------------
# roots above thresh = -1, then kept at dl = 0, 1, 2, 5: without a mask, and among the grid maxima of root NMS sz = 2
PINNED = {(48, 64): ((446, [22, 7, 4, 2]), (22, [22, 9, 6, 3])),
          (96, 128): ((2422, [87, 27, 19, 15]), (87, [87, 40, 30, 24]))}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", T.SHAPES, ids=["48x64", "96x128"])
def test_pinned_counts_on_real_frames(oracle, shape, dtype):
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat, ks = model.flatten(), T.root_ksizes(model)
    levels = T.frame_levels(oracle, flat, synth.synthetic_frame(5, shape[0], shape[1], 3), dtype)
    for masked, (roots, kept) in zip((False, True), PINNED[shape]):
        lv = T.with_root_nms(levels, flat.thresh, 2) if masked else levels
        got = []
        for dl in T.DLS:
            rec, sc, keep = both_forms(lv, ks, flat.thresh, dl)
            assert len(rec) == roots
            got.append(int(keep.sum()))
        assert got == kept, (masked, got)
        if not masked and shape == (48, 64):
            check_properties(rec, sc, keep, T.DLS[-1])


def test_plane_records_are_the_oracles_records(oracle):
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat, ks = model.flatten(), T.root_ksizes(model)
    im = synth.synthetic_frame(5, 48, 64, 3)
    levels = T.frame_levels(oracle, flat, im, np.float32)
    rec, _ = S.plane_records(levels, ks, T.eligible_planes(levels, flat.thresh))
    det = oracle.detect(flat, im)
    assert len(det) == len(rec) == 446
    for d, r in zip(det, rec):
        assert (d["level"], d["component"], d["root_x"], d["root_y"]) == (r[2], r[1], r[3], r[4])
        assert tuple(d["parts"][0]) == tuple(r[8:12])
        assert np.float32(d["score"]) == r[5:6].view(np.float32)[0]


def test_constant_frame_reaches_cross_level_ties(oracle):
    """every one of the 446 cells is eligible; interior scores repeat exactly across cells and levels"""
    model = M.synthetic_tiny_model(thresh=-1e30)
    flat, ks = model.flatten(), T.root_ksizes(model)
    levels = T.frame_levels(oracle, flat, T.constant_frame(), np.float32)
    pairs, survivors = [], []
    for dl in (0, 1, 2):
        rec, sc, keep = both_forms(levels, ks, flat.thresh, dl)
        assert len(rec) == 446 == sum(v.size for L in levels for v in L.rootv)
        total, cross = T.tied_neighbour_pairs(rec, dl)
        assert (cross > 0) == (dl > 0)
        # the ties decide: handing them to the later root gives another result
        assert not np.array_equal(T.keep_mutant(rec, dl, "tie_to_later"), keep)
        pairs.append(total)
        survivors.append(int(keep.sum()))
    assert pairs == [266, 530, 566] and survivors == [15, 4, 3]


# ---- symbols and refusals that need no GPU ---------------------------------------------------------------------------------
def test_symbols_and_null_handle_refusals():
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = _lib.load()
    for n in ["pbd_set_scale_nms", "pbd_scale_nms", "pbd_scale_nms_device"]:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert _lib.KERNELS[-1] == "k_depth_prune" and _lib.KERNELS_SCALE_NMS == ["k_scale_nms"]
    i = len(_lib.KERNELS) + len(_lib.KERNELS_MM)
    lib.pbd_kernel_name.restype = C.c_char_p
    assert lib.pbd_kernel_name(i).decode() == "k_scale_nms" and lib.pbd_kernel_name(i - 1).decode() == "k_mm_decode"
    assert lib.pbd_kernel_name(i + 1).decode() == "?"
    n = C.c_int(5)
    assert lib.pbd_set_scale_nms(None, 1, 1) == -1
    assert lib.pbd_scale_nms(None, 1, 1, None, 0, 0, None, 0, C.byref(n)) == -1
    assert lib.pbd_scale_nms_device(None, 1, 1, None, 0, 0, None, 0) == -1


def test_detector_refuses_bad_parameters_before_any_handle():
    from partsbaseddetector_amd import detector
    from partsbaseddetector_amd.detector import PbdError
    det = detector.PartsBasedDetector.__new__(detector.PartsBasedDetector)
    det.hd, det._scale_nms = None, None
    for dl in (-1, 256):
        with pytest.raises(PbdError):
            det.setScaleNMS(dl)
    det.setScaleNMS(0)
    assert det._scale_nms == 0          # dl = 0 is on: kept for distributeModel
    det.setScaleNMS(255)
    assert det._scale_nms == 255
    det.setScaleNMS(None)
    assert det._scale_nms is None
