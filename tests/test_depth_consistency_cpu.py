"""The numpy yardstick of pbd_depth_consistency (partsbaseddetector_amd.consistency) against a literal Python transcription of
SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-95) with the project's decisions applied explicitly
(include/pbd.h): boxes clipped to the depth image, NaN samples read as 0, an empty box has no median, one-part components keep.
No GPU."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd import consistency
from partsbaseddetector_amd import model as M

STRIDE = 8 + 4 * 26


def literal(flat, records, depths, zfactor, T):
    """filterCandidatesByDepth, line by line: p from nparts-1 down to 1, break on the first inconsistent edge, push at p == 1"""
    new_candidates = []
    for rec in records:
        c = int(rec[1])
        nparts = int(flat.part_offset[c + 1] - flat.part_offset[c])
        depth = depths[int(rec[0])]
        boxes = [tuple(int(v) for v in rec[8 + 4 * j:12 + 4 * j]) for j in range(nparts)]
        if nparts == 1:                                   # project decision (the reference's loop drops these)
            new_candidates.append(rec)
            continue
        p = nparts - 1
        while p >= 1:
            gp = int(flat.part_offset[c]) + p
            ax, ay = (int(v) for v in flat.anchors[int(flat.defid[int(flat.mix_offset[gp])])])   # part.anchor(0)
            child = boxes[p]
            parent = boxes[int(flat.parentid[gp])]
            cmed = literal_median(depth, child, T)
            pmed = literal_median(depth, parent, T)
            if cmed is not None and pmed is not None:     # project decision: an empty box has no median
                if cmed > 0 and pmed > 0:
                    with np.errstate(invalid="ignore", over="ignore"):
                        diff = abs(T(cmed) - T(pmed))
                    if float(diff) > math.sqrt(float(ax) * ax + float(ay) * ay) * float(np.float32(zfactor)):
                        break
            if p == 1:
                new_candidates.append(rec)
            p -= 1
    return np.array(new_candidates, np.int32).reshape(-1, records.shape[1])


def literal_median(depth, box, T):
    """Math::median<T>(depth(box & image)): sorted(samples)[M // 2], NaN read as 0"""
    x, y, w, h = box
    rows, cols = depth.shape
    x1, y1, x2, y2 = max(x, 0), max(y, 0), min(x + w, cols), min(y + h, rows)
    vals = []
    for yy in range(y1, y2):
        for xx in range(x1, x2):
            v = T(depth[yy, xx])
            vals.append(T(0) if v != v else v)
    if not vals:
        return None
    return sorted(vals)[len(vals) // 2]


def rec_of(frame, component, parts):
    r = np.zeros(STRIDE, np.int32)
    parts = np.asarray(parts, np.int32).reshape(-1, 4)
    r[0], r[1], r[6] = frame, component, len(parts)
    r[8:8 + parts.size] = parts.ravel()
    return r


def random_depth(rng, rows, cols, dtype):
    if dtype in (np.uint8, np.uint16):
        hi = 256 if dtype == np.uint8 else 65536
        d = rng.integers(0, hi, (rows, cols)).astype(dtype)
        d[rng.random((rows, cols)) < 0.2] = 0
        return d
    d = (rng.random((rows, cols)) * 4 - 0.5).astype(dtype)
    u = rng.random((rows, cols))
    d[u < 0.1] = np.nan
    d[(u >= 0.1) & (u < 0.2)] = 0
    d[(u >= 0.2) & (u < 0.22)] = np.inf
    d[(u >= 0.22) & (u < 0.23)] = -np.inf
    d[(u >= 0.23) & (u < 0.25)] = -0.0
    # coarse plateaus so that medians agree often enough for both outcomes to occur
    d[: rows // 2, : cols // 2] = dtype(1.25)
    return d


@pytest.fixture(scope="module")
def tiny():
    return M.synthetic_tiny_model().flatten()


@pytest.fixture(scope="module")
def person():
    return M.synthetic_person_model().flatten()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
def test_mirror_equals_literal_randomised(tiny, T, dtype):
    rng = np.random.default_rng(1000 + (T == np.float64) * 7 + np.dtype(dtype).num)
    depths = [random_depth(rng, 24, 30, dtype) for _ in range(3)]
    recs = []
    for i in range(1100):
        parts = [(int(rng.integers(-8, 34)), int(rng.integers(-8, 28)), int(rng.integers(-2, 12)), int(rng.integers(-2, 12)))
                 for _ in range(3)]
        recs.append(rec_of(i % 3, 0, parts))
    recs = np.stack(recs)
    z = float(rng.choice([0.03, 0.3, 3.0, 30.0]))
    for zf in (0.03, z, 1000.0 if dtype == np.uint16 else 0.5):
        want = literal(tiny, recs, depths, zf, T)
        got = consistency.filter_records(tiny, recs, depths, zf, T)
        assert np.array_equal(got, want)
    # both outcomes occur on this data
    kept = len(consistency.filter_records(tiny, recs, depths, 0.3, T))
    assert 0 < kept < len(recs)


def test_person_model_randomised(person):
    rng = np.random.default_rng(7)
    depths = [random_depth(rng, 60, 80, np.float32)]
    recs = np.stack([rec_of(0, 0, [(int(rng.integers(-10, 80)), int(rng.integers(-10, 60)), int(rng.integers(1, 20)),
                                     int(rng.integers(1, 20))) for _ in range(26)]) for _ in range(120)])
    for T in (np.float32, np.float64):
        assert np.array_equal(consistency.filter_records(person, recs, depths, 0.03, T), literal(person, recs, depths, 0.03, T))


def test_border_and_outside_boxes(tiny):
    d = np.full((10, 10), 2.0, np.float32)
    d[:, 8:] = 5.0
    recs = np.stack([
        rec_of(0, 0, [(0, 0, 4, 4), (8, 0, 10, 10), (2, 2, 2, 2)]),        # child clipped to the 5.0 strip: rejected
        rec_of(0, 0, [(0, 0, 4, 4), (20, 20, 5, 5), (2, 2, 2, 2)]),        # child fully outside: no median, kept
        rec_of(0, 0, [(-5, -5, 7, 7), (-100, 0, 102, 3), (2, 2, 2, 2)]),   # partly outside, both 2.0
        rec_of(0, 0, [(0, 0, 0, 4), (8, 0, 2, 2), (0, 0, 3, 3)]),          # empty parent: its edges are not tested
    ])
    got = consistency.filter_records(tiny, recs, [d], 0.03, np.float32)
    assert np.array_equal(got, recs[[1, 2, 3]])
    assert np.array_equal(got, literal(tiny, recs, [d], 0.03, np.float32))


def test_nan_heavy_and_even_odd_counts(tiny):
    d = np.full((8, 8), np.nan, np.float64)
    d[0, 0:3] = [1.0, 3.0, 9.0]                   # a 1 x 4 box: samples 1, 3, 9, NaN->0 -> sorted 0 1 3 9, index 2 = 3
    box_even = (0, 0, 4, 1)
    box_odd = (0, 0, 3, 1)                        # 1 3 9 -> index 1 = 3
    assert consistency.median(consistency.samples(d, box_even, np.float64)) == 3.0
    assert consistency.median(consistency.samples(d, box_odd, np.float64)) == 3.0
    assert consistency.median(consistency.samples(d, (4, 4, 3, 3), np.float64)) == 0.0   # all NaN: median 0, no test
    recs = np.stack([rec_of(0, 0, [box_even, (4, 4, 3, 3), box_odd]), rec_of(0, 0, [box_even, box_odd, (0, 0, 2, 1)])])
    for T in (np.float32, np.float64):
        want = literal(tiny, recs, [d], 0.03, T)
        assert np.array_equal(consistency.filter_records(tiny, recs, [d], 0.03, T), want)
    # record 1: parts 1 (median 3) and 2 (samples 1, 3 -> upper median 3) against part 0 (3): kept
    assert len(consistency.filter_records(tiny, recs, [d], 0.03, np.float32)) == 2


def test_infinities_and_negatives(tiny):
    d = np.zeros((4, 12), np.float32)
    d[:, 0:4] = np.inf
    d[:, 4:8] = -1.0
    d[:, 8:12] = 2.0
    inf, neg, two = (0, 0, 4, 4), (4, 0, 4, 4), (8, 0, 4, 4)
    recs = np.stack([rec_of(0, 0, [inf, inf, inf]),     # Inf - Inf = NaN: not rejected
                     rec_of(0, 0, [inf, two, two]),     # |2 - Inf| = Inf: rejected
                     rec_of(0, 0, [neg, two, two]),     # parent <= 0: not tested
                     rec_of(0, 0, [two, neg, two])])    # child <= 0: not tested
    got = consistency.filter_records(tiny, recs, [d], 0.03, np.float32)
    assert np.array_equal(got, recs[[0, 2, 3]])
    assert np.array_equal(got, literal(tiny, recs, [d], 0.03, np.float32))


def test_one_part_component_keeps():
    flat = M.synthetic_model(seed=5, pa=[0], nmix=1, name="one").flatten()
    d = np.arange(100, dtype=np.float32).reshape(10, 10)
    recs = np.stack([rec_of(0, 0, [(0, 0, 3, 3)]), rec_of(0, 0, [(50, 50, 3, 3)])])
    assert np.array_equal(consistency.filter_records(flat, recs, [d], 0.03, np.float32), recs)
    assert np.array_equal(literal(flat, recs, [d], 0.03, np.float32), recs)


def float_double_scene(flat):
    """a 64F depth with two plateaus a and b whose difference straddles the threshold of part 1's edge differently in float
    and in double: (depth, record, zfactor)"""
    norm = consistency.anchor_norms(flat)[1]
    z = 0.03
    thr = norm * float(np.float32(z))
    a = 1.0
    for k in range(-400, 400):
        b = a + thr + k * 2.0 ** -40
        f_rej = float(abs(np.float32(b) - np.float32(a))) > thr
        d_rej = abs(b - a) > thr
        if f_rej != d_rej:
            break
    else:
        raise AssertionError("no straddling value found")
    d = np.full((4, 8), a, np.float64)
    d[:, 4:] = b
    return d, rec_of(0, 0, [(0, 0, 4, 4), (4, 0, 4, 4), (0, 0, 4, 4)]), z, (f_rej, d_rej)


def test_float_and_double_round_the_difference_differently(tiny):
    d, rec, z, (f_rej, d_rej) = float_double_scene(tiny)
    recs = rec[None]
    for T, rej in ((np.float32, f_rej), (np.float64, d_rej)):
        got = consistency.filter_records(tiny, recs, [d], z, T)
        assert len(got) == (0 if rej else 1)
        assert np.array_equal(got, literal(tiny, recs, [d], z, T))


def test_negative_zero_equals_zero(tiny):
    d = np.array([[-0.0, 0.0, 0.0, -0.0]], np.float32)
    assert float(consistency.median(consistency.samples(d, (0, 0, 4, 1), np.float32))) == 0.0
