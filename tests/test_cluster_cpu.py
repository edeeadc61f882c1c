"""cluster_parts_ref (partsbaseddetector_amd/trainmodel.py), the yardstick of pbd_cluster_parts, on the built cases of
tests/cluster_cases.py: each rule of include/pbd.h's contract decides a result here, and a rule changed alone changes it.  Then
the host steps of the trainmodel pipeline (initmodel, point_to_box, data_def, merge_models, build_model) on hand-made inputs."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd import synth
from partsbaseddetector_amd import trainmodel as TM
from partsbaseddetector_amd.qp import reduce_r, reduce_seq

import cluster_cases as CC


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def trial_runs(name, part=1, R=reduce_r):
    """every trial of one part of a case, run on its own: [(labels, centres, counts, sumdist, iterations)]"""
    d, parent, K, kw, _ = CC.case(name)
    P, N = d.shape[:2]
    start = (synth.splitmix64(kw["seed"], P * kw["trials"] * 16) % np.uint64(N)).astype(np.int64).reshape(P, kw["trials"], 16)
    X = TM.offsets(d, np.asarray(parent), part)
    return [TM.k_means_ref(X, start[part, r, :K[part]], kw["max_iter"], R) for r in range(kw["trials"])]


def test_grid_ties_pick_the_first():
    _, _, _, _, want = CC.case("grid")
    runs = trial_runs("grid")
    sd = np.array([r[3] for r in runs])
    assert sd.tobytes() == want["sumdist_all"][1].tobytes()
    best = int(want["info"][1]["best_trial"])
    tied = [r for r in range(len(sd)) if sd[r] == sd.min()]
    assert len({tuple(runs[r][0]) for r in tied}) >= 2, "the minimum is reached by one labeling only: the case pins nothing"
    assert best == tied[0] and len(tied) >= 2
    assert np.array_equal(want["idx"][1], runs[best][0])
    # the last of the tied trials is another partition: a pick by <= instead of < changes idx
    assert not np.array_equal(runs[tied[-1]][0], runs[best][0]) or len({tuple(runs[r][0]) for r in tied[:-1]}) >= 2


def test_duplicate_points_leave_nan_centres_and_every_point_labelled(monkeypatch):
    d, parent, K, kw, want = CC.case("dup")
    runs = trial_runs("dup")
    for g, c, counts, sd, it in runs:
        assert np.isnan(c).any() and it <= 2
        assert g.min() >= 0 and counts.sum() == d.shape[1] and sd == sd
        assert np.array_equal(np.isnan(c[:, 0]), counts == 0)
    assert np.isnan(want["centres"][1, :4]).any() and not np.isnan(want["centres"][1, :4]).all()
    assert np.isnan(want["centres"][1, 4:]).all() and not want["counts"][1, 4:].any()
    assert np.array_equal(want["anchors"][1][want["counts"][1] == 0], np.zeros((int((want["counts"][1] == 0).sum()), 2)))

    def nan_wins(X, c):   # the mutation: a NaN distance counts as the smallest
        label = np.full(len(X), -1, np.int64)
        z = np.full(len(X), np.inf)
        for t in range(len(c)):
            dx, dy = X[:, 0] - c[t, 0], X[:, 1] - c[t, 1]
            D = (0.0 + dx * dx) + dy * dy
            D = np.where(np.isnan(D), -1.0, D)
            take = (label < 0) | (D < z)
            label[take], z[take] = t, D[take]
        return label, z
    monkeypatch.setattr(TM, "_labels", nan_wins)
    got = TM.cluster_parts_ref(d, parent, K, **kw)
    assert not np.array_equal(got["idx"], want["idx"]) or got["sumdist_all"].tobytes() != want["sumdist_all"].tobytes()


@pytest.mark.parametrize("name", ["order257", "order1000"])
def test_summation_order_decides_centre_bits(name):
    d, parent, K, kw, want = CC.case(name)
    lit = TM.cluster_parts_ref(d, parent, K, literal=True, **kw)
    a, b = trial_runs(name, R=reduce_r), trial_runs(name, R=reduce_seq)
    differ = sum(bits(x[1]).tobytes() != bits(y[1]).tobytes() for x, y in zip(a, b))
    assert differ >= 1
    assert lit["sumdist_all"].tobytes() != want["sumdist_all"].tobytes()
    assert np.array_equal(lit["counts"].sum(axis=1), want["counts"].sum(axis=1))


def test_single_member_type_keeps_its_member():
    d, parent, K, kw, want = CC.case("single")
    X = TM.offsets(d, np.asarray(parent), 1)
    counts = want["counts"][1, :2]
    assert sorted(counts) == [1, 3]
    t = int(np.argmin(counts))
    assert bits(want["centres"][1, t]).tobytes() == bits(X[3]).tobytes()          # (40, 7), not (23.5, 23.5)
    assert tuple(want["anchors"][1, t]) == (40, 7)
    assert int(want["idx"][1, 3]) == t and not np.any(want["idx"][1, :3] == t)


def test_anchor_rounding_is_matlabs_round_of_centre_plus_one():
    d, parent, idx, K = CC.halves()
    c = TM.centres_of(d, parent, idx, K)
    assert c[1, :4, 0].tolist() == [2.5, -0.5, -1.5, -2.5] and c[1, :4, 1].tolist() == [-2.5, -1.5, -0.5, 2.5]
    assert np.isnan(c[1, 4:]).all() and np.isnan(c[0, 1:]).all()
    a = TM.anchors_of(c)
    assert a[1, :4, 0].tolist() == [3, 0, -2, -3] and a[1, :4, 1].tolist() == [-3, -2, 0, 3]
    assert not a[0].any() and not a[1, 4:].any()
    assert [TM.anchor_of(v) for v in (0.5, 1.5, -1.0, float("nan"), 1e300, -1e300, float("inf"))] == \
        [1, 2, -1, 0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]
    # round(c), halves away from zero, differs exactly where c + 1 crosses zero's side: -0.5 -> -1, the rule gives 0
    away = lambda v: int(math.copysign(math.floor(abs(v) + 0.5), v))
    assert [away(v) for v in (2.5, -0.5, -1.5, -2.5)] == [3, -1, -2, -3]


def test_root_clusters_its_lowest_childs_offsets():
    d, parent, K, kw, want = CC.case("tree")
    two = TM.cluster_parts_ref(d[:2], parent[:2], K[:2], **kw)
    assert np.array_equal(want["idx"][0], two["idx"][0]) and np.array_equal(want["idx"][1], two["idx"][1])
    assert bits(want["centres"][0]).tobytes() == bits(two["centres"][0]).tobytes()
    assert not want["anchors"][0].any()
    # the groups are the built ones: parity of n for parts 0 and 1, n % 4 < 2 for part 2, n % 5 == 0 for part 3
    n = np.arange(d.shape[1])
    for p, built in ((0, n % 2), (1, n % 2), (2, (n % 4 < 2).astype(int)), (3, (n % 5 == 0).astype(int))):
        g = want["idx"][p]
        assert np.array_equal(g, built) or np.array_equal(g, 1 - built), p
    # part 3 hangs off part 2: its anchors are those of +-6.25 (6 and -6), not of its offset to the root (+-6.25 +-12)
    assert sorted(want["anchors"][3, :2, 0].tolist()) == [-6, 6]
    other = TM.cluster_parts_ref(np.stack([d[0], d[2]]), [-1, 0], [2, 2], **kw)
    assert not np.array_equal(other["idx"][0], want["idx"][0])


def test_max_iter_cuts_a_trial_while_labels_change():
    d, parent, K, kw, full = CC.case((1025,))
    for cut in (1, 2):
        got = TM.cluster_parts_ref(d, parent, K, **dict(kw, max_iter=cut))
        assert got["iters_all"].max() == cut and np.all(got["iters_all"][full["iters_all"] > cut] == cut)
        assert np.any(full["iters_all"] > cut)
    assert np.all(TM.cluster_parts_ref(d, parent, K, **dict(kw, max_iter=1))["iters_all"] == 1)


def test_pick_skips_nan_and_defaults_to_trial_zero():
    nan = float("nan")
    assert TM.pick_trial([nan, 3.0, 2.0, 2.0, nan]) == 2
    assert TM.pick_trial([nan, nan]) == 0 and TM.pick_trial([1.0, 1.0]) == 0


@pytest.mark.parametrize("bad", [
    dict(d=np.zeros((1, 4, 2)), parent=[-1], K=[1]),
    dict(K=[0, 2]), dict(K=[2, 17]), dict(trials=0), dict(max_iter=0), dict(parent=[0, 0]), dict(parent=[-1, 1]), dict(parent=[-1, -1]),
    dict(d=np.zeros((2, 0, 2)))])
def test_invalid_arguments_raise(bad):
    kw = dict(d=np.zeros((2, 4, 2)), parent=[-1, 0], K=[2, 2], trials=2, max_iter=5)
    kw.update(bad)
    with pytest.raises(ValueError):
        TM.cluster_parts_ref(kw["d"], kw["parent"], kw["K"], kw["trials"], kw["max_iter"], 0)


# ---- the pipeline's host steps ---------------------------------------------------------------------------------------------------
def _square_pos(side, pts=((10.0, 10.0),)):
    return {"im": None, "points": np.array(pts), "boxes": np.array([[0, 0, side - 1, side - 1]] * len(pts))}


@pytest.mark.parametrize("n,index", [(1, 1), (19, 1), (20, 1), (40, 2)])
def test_initmodel_percentile_index(n, index):
    assert TM.percentile_index(n) == index
    sides = [8 * (n - i) + 8 for i in range(n)]                 # descending: the sort matters
    pos = [_square_pos(s) for s in sides]
    m = TM.initmodel(pos, sbin=4)
    k = sorted(sides)[index - 1] // 4
    assert m.filtersw[0].shape == (k, k * 32) and not m.filtersw[0].any() and m.biasw == [0.0]
    assert (m.filterid, m.biasid, m.defid, m.parentid, m.interval, m.sbin) == ([[[0]]], [[[0]]], [[[]]], [[-1]], 10, 4)
    m.validate()
    assert TM.initmodel(pos, sbin=4, tsize=5).filtersw[0].shape == (5, 160)
    with pytest.raises(ValueError):
        TM.initmodel([_square_pos(3)], sbin=4)


def test_point_to_box_by_hand():
    pts = np.array([[(0, 0), (3, 4), (3, 14)], [(0, 0), (6, 8), (6, 38)]], np.float64)    # limbs 5, 10 and 10, 30
    r2 = math.exp((math.log(10 / 5) + math.log(30 / 10)) / 2)                               # the median of two is their mean
    sizes = []
    for l1, l2 in ((5.0, 10.0), (10.0, 30.0)):
        lo, hi = sorted([l1 / 1.0, l2 / r2])
        sizes.append(lo + 0.85 * (hi - lo))                                                 # quantile(., 0.85), method 7, two samples
    got = TM.point_to_box(pts, [0, 1, 2])
    assert got.shape == (2, 3, 4)
    for n in range(2):
        for p in range(3):
            x, y = pts[n, p]
            assert np.allclose(got[n, p], [x - sizes[n] / 2, y - sizes[n] / 2, x + sizes[n] / 2, y + sizes[n] / 2], rtol=0, atol=1e-12)
    assert TM.round_boxes([[0.5, -0.5, 2.5, -2.5, 2.4999]]).tolist() == [[1, -1, 3, -3, 2]]
    pos = TM.with_boxes([{"im": None, "points": pts[0]}, {"im": None, "points": pts[1], "boxes": np.zeros((3, 4))}], [0, 1, 2])
    assert np.array_equal(pos[0]["boxes"], TM.round_boxes(got[0])) and not pos[1]["boxes"].any()


def test_data_def_scales_by_the_root_box():
    pos = [_square_pos(20, [(10.0, 30.0), (14.0, 2.0)]), _square_pos(40, [(10.0, 30.0), (14.0, 2.0)])]
    d = TM.data_def(pos, 5)
    assert d.shape == (2, 2, 2) and d.flags["C_CONTIGUOUS"]
    assert d[0, 0].tolist() == [10 / 4, 30 / 4] and d[1, 1].tolist() == [14 / 8, 2 / 8]


def _part_model(k, values):
    ms = []
    for v in values:
        m = TM.initmodel([_square_pos(40)], 4, tsize=k)
        m.filtersw[0][:] = v
        m.biasw[0] = 0.25
        ms.append(m)
    return TM.merge_models(ms)


def test_merge_and_build_model_tables():
    init = TM.initmodel([_square_pos(40)], 4, tsize=3, interval=10)
    parts = [_part_model(3, [1, 2]), _part_model(3, [3, 4, 5]), _part_model(3, [6])]
    assert parts[1].ncomponents() == 3 and parts[1].filterid == [[[0]], [[1]], [[2]]] and parts[1].biasid == [[[0]], [[1]], [[2]]]
    assert parts[1].parentid == [[-1]] * 3 and parts[1].defid == [[[]]] * 3
    idx = [np.array([0, 1, 0, 1]), np.array([0, 1, 2, 2]), np.array([0, 0, 0, 0])]
    anchors = np.zeros((3, 16, 2), np.int32)
    anchors[1, :3] = [(1, -2), (3, 4), (-5, 6)]
    anchors[2, 0] = (7, 8)
    m = TM.build_model(init, parts, idx, anchors, [2, 3, 1], [0, 1, 1])
    m.validate()
    assert m.ncomponents() == 1 and m.parentid == [[-1, 0, 0]]
    assert m.filterid == [[[0, 1], [2, 3, 4], [5]]] and m.defid == [[[], [0, 1, 2], [3]]]
    assert m.biasid == [[[0], [1 + k * 2 + l for l in range(2) for k in range(3)], [7 + l for l in range(2)]]]
    assert m.biasid[0][1] == [1, 3, 5, 2, 4, 6]
    assert m.biasw == [0.0] * 9 and m.defw == [[0.01, 0.0, 0.01, 0.0]] * 4
    assert m.anchors == [(1, -2), (3, 4), (-5, 6), (7, 8)]
    assert [float(f[0, 0]) for f in m.filtersw] == [1, 2, 3, 4, 5, 6]
    assert (m.interval, m.sbin, m.thresh) == (10, 4, 0.0)
    assert len(m.to_vector()) == 9 + 4 * 4 + 6 * 3 * 3 * 32
    flat = m.flatten()
    assert flat.biasid.tolist() == [0, -1, 1, 3, 5, 7] and flat.defid.tolist() == [-1, -1, 0, 1, 2, 3]
    # centres instead of anchors go through the rounding rule
    centres = np.full((3, 16, 2), np.nan)
    centres[1, :3] = [(0.5, -2.5), (2.6, 3.5), (-5.5, 6.0)]
    centres[2, 0] = (-0.5, 8.4)
    assert TM.build_model(init, parts, idx, centres, [2, 3, 1], [0, 1, 1]).anchors == [(1, -3), (3, 4), (-6, 6), (0, 8)]
    with pytest.raises(ValueError, match="part 1 type 2"):
        TM.build_model(init, parts, [idx[0], np.array([0, 1, 1, 1]), idx[2]], anchors, [2, 3, 1], [0, 1, 1])
    with pytest.raises(ValueError):
        TM.build_model(init, parts, idx, anchors, [2, 3, 1], [0, 2, 1])
