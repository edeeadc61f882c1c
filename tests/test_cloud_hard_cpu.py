"""The built hard clouds of tests/cloud_hard_scenes.py, checked on the CPU alone: every scene reaches what it is named for (asserted
from the numpy yardstick, partsbaseddetector_amd/pointcloud.py), the yardstick equals the literal restatements of
tests/test_planes_cpu.py and tests/test_pointcloud_cpu.py on the small ones, and the yardstick with any single rule changed gives
another result on a named scene -- so a kernel with that rule changed fails tests/test_gpu_cloud_hard.py.  No GPU is used here."""
import contextlib
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

import cloud_hard_scenes as S
from partsbaseddetector_amd import pointcloud as pc
from partsbaseddetector_amd.pointcloud import PointCloudClusterer as PCC

F = np.float32


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_literal", os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LP = _load("test_planes_cpu")          # literal_normal, literal_segments, literal_refine, pre_refine
LC = _load("test_pointcloud_cpu")      # literal_cluster


@functools.lru_cache(maxsize=None)
def plane_calls(family):
    return S.PLANE_SCENES[family]()


@functools.lru_cache(maxsize=None)
def cluster_calls(family):
    return S.CLUSTER_SCENES[family]()


def plane_result(call):
    with np.errstate(all="ignore"):
        return [PCC.organizedMultiplaneSegmentation(c, call.params) for c in call.clouds]


def plane_state(call):
    return tuple((r[2].tobytes(), r[3].tobytes(), r[1].tobytes()) for r in plane_result(call))


def cluster_state(call):
    cen, idx = PCC.clusterObjects(call.clouds, call.boxes, call.frames)
    return cen.tobytes(), tuple(tuple(int(v) for v in i) for i in idx)


@functools.lru_cache(maxsize=None)
def plane_reference(family, name):
    return plane_result(plane_calls(family)[name])


@functools.lru_cache(maxsize=None)
def cluster_reference(family, name):
    call = cluster_calls(family)[name]
    return PCC.clusterObjects(call.clouds, call.boxes, call.frames)


def passes(P, q):
    """(labels before refinement, after the forward pass, after the backward pass, planes, roots)"""
    with np.errstate(all="ignore"):
        _, _, root, lab, planes = LP.pre_refine(P, q)
        if not len(planes):
            return lab, lab, lab, planes, root
        fwd = pc.plane_refine_pass(lab, P, planes, q.distance_threshold)
        bwd = pc.plane_refine_pass(fwd[::-1, ::-1], P[::-1, ::-1], planes, q.distance_threshold)[::-1, ::-1]
    return lab, fwd, bwd, planes, root


def candidates(P, q):
    """the roots of the finite segments above min_inliers"""
    with np.errstate(all="ignore"):
        _, _, root, _, _ = LP.pre_refine(P, q)
    fin = np.isfinite(P[:, :, :3]).all(axis=2).ravel()
    size = np.bincount(root[fin], minlength=len(root))
    return np.nonzero((size > q.min_inliers) & fin & (root == np.arange(len(root))))[0], root


# ---- reach: planes ------------------------------------------------------------------------------------------------------------
def test_tall_clouds_cross_the_lds_exchange_and_refinement_relabels_them():
    calls = plane_calls("tall")
    assert calls["4097x13"].clouds[0].shape[:2] == (S.REF_LDS_ROWS + 1, 13)
    assert calls["4100x24"].clouds[0].shape[:2] == (S.REF_LDS_ROWS + 4, 24)
    rows = [c.shape[0] for c in calls["small_4100_4097"].clouds]
    assert rows[0] <= S.REF_LDS_ROWS and rows[1] > S.REF_LDS_ROWS and rows[2] > S.REF_LDS_ROWS     # both tall ones at rbase != 0
    assert [c.shape[0] for c in calls["1024x16_1025x16"].clouds] == [S.REF_THREADS, S.REF_THREADS + 1]
    for name in ("4097x13", "4100x24"):
        call = calls[name]
        lab, fwd, bwd, planes, _ = passes(call.clouds[0], call.params)
        assert len(planes) >= 1
        assert (fwd != lab).sum() > 10000 and (bwd != fwd).sum() > 10000            # each pass decides labels
    lab, fwd, bwd, _, _ = passes(calls["4100x24"].clouds[0], calls["4100x24"].params)
    assert (bwd != lab).sum() > 45000


def test_snake_segments_hook_far_from_their_root():
    for name, call in plane_calls("snake").items():
        P = call.clouds[0]
        (res,) = plane_reference("snake", name)
        assert len(res[3]) == 1                                      # one segment through every corridor
        cand, root = candidates(P, call.params)
        assert len(cand) == 1
        H, W = P.shape[:2]
        member = np.nonzero(root == cand[0])[0]
        rows, cols = member // W, member % W
        assert rows.max() - rows.min() > 0.9 * H - 12 and cols.max() - cols.min() > 0.9 * W - 12
        # a raster two-pass labelling needs many provisional labels for it: members with neither a left nor an upper member
        m = (root == cand[0]).reshape(H, W)
        starts = m & ~np.pad(m, ((0, 0), (1, 0)))[:, :-1] & ~np.pad(m, ((1, 0), (0, 0)))[:-1]
        assert starts.sum() >= 10


def test_singles_more_candidates_than_workgroups_and_64_roots_in_a_wave():
    call = plane_calls("singles")["checker_70x70"]
    cand, root = candidates(call.clouds[0], call.params)
    assert len(cand) == 4900 > S.MAX_GRID
    assert np.array_equal(root, np.arange(4900))                     # every 64 consecutive points: 64 distinct roots
    (res,) = plane_reference("singles", "checker_70x70")
    assert len(res[3]) == 0 and len(res[1]) == 4900 and res[1][-1] == 4899        # 0/0 curvature: no plane; the last point kept
    call = plane_calls("singles")["patches_15x15"]
    (res,) = plane_reference("singles", "patches_15x15")
    assert len(res[3]) == 225 > 64                                   # above the default capacity guess of Handle.remove_planes
    lab, fwd, bwd, planes, root = passes(call.clouds[0], call.params)
    assert (np.bincount(lab[lab >= 0]) == 9).all()                   # 3 x 3 cores
    # the rings absorbed, forward and backward; a patch on the image's first row keeps its upper left corner: in the backward
    # pass that is the last row (no label from the side), and the point diagonally beside it is NaN (none from below)
    assert np.array_equal(np.bincount(bwd[bwd >= 0]), [48] * 15 + [49] * 210)
    assert (fwd != lab).any() and (bwd != fwd).any()
    assert len(np.unique(planes[:, 3])) == 225


def other_orders():
    seq = pc.moment_total
    return {"pairwise": lambda v: float(np.sum(v)),
            "columns first": lambda v: seq(np.ascontiguousarray(v.T)),
            "right to left, bottom to top": lambda v: seq(v[::-1, ::-1])}


@contextlib.contextmanager
def changed(hook, value):
    old = getattr(pc, hook)
    setattr(pc, hook, value)
    try:
        yield
    finally:
        setattr(pc, hook, old)


def test_far_coefficients_depend_on_the_order_of_the_moment_sums():
    call = plane_calls("far")["far"]
    P = call.clouds[0]
    assert P.shape[0] > S.MOMENT_ROWS and P.shape[1] > 64 and 350 < abs(P[..., 0]).min()
    (res,) = plane_reference("far", "far")
    assert len(res[3]) == 1
    for name, order in other_orders().items():
        with changed("moment_total", order):
            (other,) = plane_result(call)
        assert np.array_equal(other[2], res[2]) and other[3].tobytes() != res[3].tobytes(), name
    # near the axis no order shows: the reason this scene exists
    near = S.PlaneCall([S.sheet(200, 300, 2.0, 0.05, 0.02)], call.params)
    (base,) = plane_result(near)
    for name, order in other_orders().items():
        with changed("moment_total", order):
            assert plane_result(near)[0][3].tobytes() == base[3].tobytes()


def test_edges_shapes_counts_and_special_values():
    calls = plane_calls("edges")
    want = {"flat_1023": 1, "flat_1024": 1, "flat_1025": 1, "flat_2048": 1, "flat_2049": 0, "flat_2049T": 0}
    for name, planes in want.items():
        n = int(name.split("_")[1].rstrip("T"))
        for kind in ("flat", "checker"):
            c = calls[name.replace("flat", kind)].clouds[0]
            assert c.shape[0] * c.shape[1] == n
        assert len(plane_reference("edges", name)[0][3]) == planes
        kept = plane_reference("edges", name.replace("flat", "checker"))[0][1]
        assert len(kept) == n and kept[-1] == n - 1                 # the last point is a one-point candidate and is kept
    assert {1023, 1024, 1025, 2048, 2049} == {S.SCAN_TILE - 1, S.SCAN_TILE, S.SCAN_TILE + 1, 2 * S.SCAN_TILE, 2 * S.SCAN_TILE + 1}
    res = plane_reference("edges", "around_2s+3")
    assert [len(r[3]) for r in res] == [0, 1, 0, 1, 0, 0]           # 12: no valid centre; 13: one row or column of them
    call = calls["collinear"]
    sizes = []
    for c in call.clouds:
        cand, root = candidates(c, call.params)
        sizes.append(int(np.bincount(root).max()))
    assert sizes == [1, 2, 3, 5, 2, 3, 1, 1]                          # one point, two and three collinear points, ...
    assert [c.shape[1] for c in calls["ballot_tiles"].clouds] == [64, 65, 63]
    assert [c.shape[0] for c in calls["moment_rounds"].clouds] == [S.MOMENT_ROWS, S.MOMENT_ROWS + 1, 2 * S.MOMENT_ROWS + 1]
    assert all(len(r[3]) == 1 for r in plane_reference("edges", "ballot_tiles") + plane_reference("edges", "moment_rounds"))
    P = calls["special_values"].clouds[0]
    assert np.isinf(P).sum() >= 2 and (P[..., 2] == 0).sum() >= 2 and (P[..., 2] < 0).any()
    with np.errstate(all="ignore"):
        assert np.isinf(P[15, 15] * P[15, 15]).all() and np.isfinite(P[15, 15]).all()
    (res,) = plane_reference("edges", "special_values")
    assert len(res[3]) == 1 and res[2][15, 15] == -1 and res[2][9, 9] == -1


def test_refine_scenes_each_guard_decides_its_point():
    calls = plane_calls("refine")
    lab = {name: plane_reference("refine", name)[0][2] for name in calls}
    assert lab["upper_right_nan"][10, 9] == -1 and lab["upper_right_nan"][9, 9] == 0
    assert lab["upper_right_finite"][10, 8] == 0
    assert lab["last_column"][10, 11] == -1 and lab["last_column"][9, 11] == 0
    assert lab["last_row"][11, 10] == -1 and lab["last_row"][11, 9] == 0 and lab["last_row"][10, 10] == -1
    two = lab["upper_beats_left"]
    A, B = two[5, 16], two[10, 6]
    assert A >= 0 and B >= 0 and A != B and two[11, 16] == A
    assert two[10, 16] == A and two[11, 15] == B                     # both neighbours of X carry their planes
    call = calls["upper_beats_left"]
    _, fwd, _, _, _ = passes(call.clouds[0], call.params)
    assert fwd[10, 16] == A and fwd[11, 15] == B and fwd[11, 16] == A        # ... already in the forward pass
    call = calls["staircase"]
    before, fwd, bwd, _, _ = passes(call.clouds[0], call.params)
    assert all(before[p] == -2 and fwd[p] == -2 and bwd[p] == 0 for p in S.STAIRS)
    t = lab["thresholds"]
    assert [t[2, 10], t[4, 10], t[6, 10], t[8, 10]] == [-1, -1, 0, 0]
    (res,) = plane_reference("refine", "thresholds")
    assert np.array_equal(res[3], np.array([[0, 0, -1, 2]], np.float32))          # the fitted plane is exact


def test_joins_hold_pairs_at_equality():
    calls = plane_calls("joins")
    for name, s in (("cos_equal", 1), ("dist_equal", 1)):
        call = calls[name]
        P, q = call.clouds[0], call.params
        with np.errstate(all="ignore"):
            N, D = pc.plane_normals(P, s, q.depth_change_factor)
        z = P[..., 2]
        a, b = (slice(None), slice(1, None)), (slice(None), slice(None, -1))
        dot = (N[a][..., 0] * N[b][..., 0] + N[a][..., 1] * N[b][..., 1]) + N[a][..., 2] * N[b][..., 2]
        dd = np.abs(D[a] - D[b])
        up, vp = (slice(1, None),), (slice(None, -1),)
        dot = np.concatenate([dot.ravel(), ((N[up][..., 0] * N[vp][..., 0] + N[up][..., 1] * N[vp][..., 1]) + N[up][..., 2] * N[vp][..., 2]).ravel()])
        dd = np.concatenate([dd.ravel(), np.abs(D[up] - D[vp]).ravel()])
        thr = np.concatenate([(F(q.distance_threshold) * (z[a] * z[a])).ravel(), (F(q.distance_threshold) * (z[up] * z[up])).ravel()])
        ok = np.isfinite(dot)
        if name == "cos_equal":
            cos_thr = F(math.cos(q.angular_threshold))
            assert (dot[ok] == cos_thr).sum() >= 1 and (dot[ok] > cos_thr).any() and (dot[ok] < cos_thr).any()
        else:
            assert (dd[ok] == thr[ok]).sum() >= 1 and (dd[ok] > thr[ok]).any() and (dd[ok] < thr[ok]).any()
    step = calls["depth_step"].clouds[0]
    z = step[..., 2]
    d = np.abs(z[:, 20] - z[:, 19])
    assert (d > F(0.02) * z[:, 19]).all() and (d <= F(0.02) * z[:, 20]).all()


def test_many_is_about_forty_mixed_clouds():
    clouds = plane_calls("many")["many"].clouds
    assert 38 <= len(clouds) <= 44
    shapes = [c.shape[:2] for c in clouds]
    assert (2, 2) in shapes and any(r == 2 and c > 2 for r, c in shapes) and any(c == 2 and r > 2 for r, c in shapes)
    tall = [i for i, (r, _) in enumerate(shapes) if r > S.REF_LDS_ROWS]
    assert tall and 5 < tall[0] < len(clouds) - 5
    assert any(np.isnan(c).all() for c in clouds)
    planes = [len(r[3]) for r in plane_reference("many", "many")]
    assert sum(p > 0 for p in planes) > 20 and max(planes) >= 2


# ---- reach: clusters ----------------------------------------------------------------------------------------------------------
def test_chain_is_one_component_in_three_orders():
    for name, call in cluster_calls("chain").items():
        cen, idx = cluster_reference("chain", name)
        assert len(idx[0]) == 20000 and np.array_equal(idx[0], np.arange(20000))
    x = cluster_calls("chain")["reversed"].clouds[0][:, 0]
    assert (np.diff(x) < 0).all()                                   # the root (index 0) is the far end: every hook is long
    x = cluster_calls("chain")["even_odd"].clouds[0][:, 0]
    assert abs(np.diff(x)[:9999] - 0.018).max() < 1e-4              # neighbours in space are 10 000 indices apart


def test_faces_every_direction_crosses_a_cell_face_at_the_radius():
    call = cluster_calls("faces")["faces"]
    P = call.clouds[0]
    cen, idx = cluster_reference("faces", "faces")
    assert len(call.boxes) == 2 * 26 * 2 * 2 and len(P) == 2 * len(call.boxes)
    cell = np.floor(P * pc.CELL_INV).astype(np.int64)
    seen = set()
    r2 = float(pc.RADIUS) * float(pc.RADIUS)
    k = 0
    for sign in (-1, 1):
        for d in S.DIRECTIONS:
            for nudge in (-1, 1):
                for partner_first in (False, True):
                    i = 2 * k
                    a, b = (i + 1, i) if partner_first else (i, i + 1)
                    assert tuple(cell[b] - cell[a]) == d, (sign, d, nudge)
                    dd = P[a] - P[b]
                    d2 = float(F(F(dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]))
                    assert (d2 <= r2) == (nudge < 0) and abs(math.sqrt(d2) - 0.01) < 2e-7
                    assert list(idx[k]) == ([i, i + 1] if nudge < 0 else [i])
                    assert np.sign(P[a][0]) == sign
                    seen.add((sign, d))
                    k += 1
    assert len(seen) == 52


def test_dense_ties_boxes_crop_edge_and_chunks_reach_their_sizes():
    call = cluster_calls("dense")["dense"]
    P = call.clouds[0]
    assert len(np.unique(np.floor(P * pc.CELL_INV), axis=0)) == 1 and len(P) == 800
    assert len(P) - len(np.unique(P, axis=0)) >= 399
    assert len(cluster_reference("dense", "dense")[1][0]) == 800
    for name, (count, size) in {"2x2": (2, 2), "3x2": (3, 2), "2x300": (2, 300), "3x300": (3, 300)}.items():
        P = cluster_calls("ties")[name].clouds[0]
        lab = PCC.components(P)
        sizes = np.bincount(lab)
        assert sorted(sizes[sizes > 0]) == [size] * count
        cen, idx = cluster_reference("ties", name)
        assert idx[0][0] == 0 and len(idx[0]) == size and (size <= 2 or idx[0][1] > len(P) - size)    # the winner finishes last
    assert 300 > S.SELECT_ROUND
    cen, idx = cluster_reference("ties", "301_300_301")
    assert len(idx[0]) == 301 and idx[0][0] == 0
    for name, n in (("300", 300), ("4200", 4200)):
        call = cluster_calls("boxes")[name]
        assert len(call.boxes) == n and len(call.clouds[0]) == 48
        counts = np.array([len(i) for i in cluster_reference("boxes", name)[1]])
        crops = np.array([len(PCC.crop(call.clouds[0], b)) for b in call.boxes[:64]])
        assert (counts == 0).sum() > n // 2 and len(np.unique(counts)) >= 5 and (crops[counts[:64] > 0] > counts[:64][counts[:64] > 0]).any()
    assert 300 > S.SELECT_ROUND and 4200 > S.MAX_GRID
    for n in (1, 2, 3):
        call = cluster_calls("boxes")["crop_%d" % n]
        assert len(PCC.crop(call.clouds[0], call.boxes[0])) == n
    for n in (S.HOST_CROP - 1, S.HOST_CROP, S.HOST_CROP + 1):
        call = cluster_calls("crop_edge")[str(n)]
        assert len(PCC.crop(call.clouds[0], call.boxes[0])) == n
        assert len(cluster_reference("crop_edge", str(n))[1][0]) == n
    for n in (1023, 1024, 1025, 2049):
        call = cluster_calls("chunks")[str(n)]
        _, on = S.chunk_cloud(n)
        assert list(cluster_reference("chunks", str(n))[1][0]) == on and list(PCC.crop(call.clouds[0], call.boxes[0])) == on
        assert 0 in on and n - 1 in on and (n <= 1024 or (1023 in on and 1024 in on))
    padded = cluster_calls("chunks")["5_floats_padded"].clouds[0]
    assert padded.shape == (33, 31, 5) and padded.strides == (40 * 20, 20, 4)


# ---- the literal restatements on the small scenes -----------------------------------------------------------------------------
SMALL_PLANES = [("refine", n) for n in ("upper_right_nan", "upper_right_finite", "last_column", "last_row", "upper_beats_left",
                                        "staircase", "thresholds")]
SMALL_PLANES += [("edges", n) for n in ("around_2s+3", "collinear", "special_values", "flat_1025", "checker_1023")]
SMALL_PLANES += [("joins", "depth_step"), ("joins", "cos_equal"), ("joins", "dist_equal")]


@pytest.mark.parametrize("family,name", SMALL_PLANES)
def test_plane_yardstick_equals_the_literal_loops(family, name):
    call = plane_calls(family)[name]
    q = call.params
    s = q.smoothing_size // 2
    rng = np.random.default_rng(1)
    for P, res in zip(call.clouds, plane_reference(family, name)):
        H, W = P.shape[:2]
        with np.errstate(all="ignore"):
            N, D = pc.plane_normals(P, s, q.depth_change_factor)
            for r, c in rng.integers(0, [H, W], size=(40, 2)):
                want = np.array(LP.literal_normal(P, r, c, s, q.depth_change_factor), np.float32)
                got = np.array([N[r, c, 0], N[r, c, 1], N[r, c, 2], D[r, c]], np.float32)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or (np.isnan(got).all() and np.isnan(want).all())
            fin = np.isfinite(P).all(axis=2)
            got = pc.plane_segments(P, N, D, q.distance_threshold, q.angular_threshold).reshape(H, W)
            want = LP.literal_segments(P, N, D, q.distance_threshold, q.angular_threshold)
            assert np.array_equal(got[fin], want[fin])
            _, _, _, lab, planes = LP.pre_refine(P, q)
            if q.refine and len(planes):
                lab = LP.literal_refine(lab, P, planes, q.distance_threshold)
        assert np.array_equal(res[2], np.where(lab >= 0, lab, -1))
        assert np.array_equal(res[1], np.nonzero(lab.ravel() < 0)[0])


SMALL_CLUSTERS = [("faces", "faces"), ("ties", "2x2"), ("ties", "3x2"), ("boxes", "300"), ("boxes", "crop_1"), ("boxes", "crop_2"),
                  ("boxes", "crop_3"), ("boxes", "crop_2_x40"), ("boxes", "on_faces"), ("chunks", "1023"), ("chunks", "1025"),
                  ("chunks", "2049"), ("chunks", "5_floats_padded"), ("dense", "dense")]


@pytest.mark.parametrize("family,name", SMALL_CLUSTERS)
def test_cluster_yardstick_equals_the_brute_force_search(family, name):
    call = cluster_calls(family)[name]
    cen, idx = cluster_reference(family, name)
    for i, box in enumerate(call.boxes):
        want_c, want_i = LC.literal_cluster(np.ascontiguousarray(call.clouds[int(call.frames[i])]), box)
        assert list(idx[i]) == want_i, i
        assert LC.same_f32(cen[i], want_c) or (np.isnan(cen[i]).all() and np.isnan(want_c).all())


# ---- one rule changed at a time -----------------------------------------------------------------------------------------------
def forward_only(lab, P, planes, dist):
    return pc.plane_refine_pass(lab, P, planes, dist)


PLANE_RULES = {
    # rule: (hook of pointcloud.py, its changed form, the scenes that must notice)
    "join threshold uses z of the neighbour": ("join_depth", lambda zp, zq: zq, [("joins", "dist_equal")]),
    "absorb threshold uses z of the absorbed point": ("absorb_depth", lambda zf, za: za, [("refine", "thresholds")]),
    "> becomes >= at cos_thr": ("parallel", lambda dot, thr: dot >= thr, [("joins", "cos_equal")]),
    "< becomes <= at the join threshold": ("join_near", lambda d, thr: d <= thr, [("joins", "dist_equal")]),
    "< becomes <= at the absorb threshold": ("absorb_near", lambda d, thr: d <= thr, [("refine", "thresholds")]),
    "depth-edge test uses z of the neighbour": ("edge_tolerance", lambda tc, tn: tn, [("joins", "depth_step")]),
    "(r-1, c+1) test dropped": ("refine_upper_right", lambda fin, r, c: np.ones(len(r), bool), [("refine", "upper_right_nan")]),
    "last-column guard dropped": ("refine_upper_column", lambda c, W: np.ones(len(c), bool), [("refine", "last_column")]),
    "last-row guard dropped": ("refine_left_row", lambda r, H: np.ones(len(r), bool), [("refine", "last_row")]),
    "left before upper": ("REFINE_ORDER", ("left", "upper"), [("refine", "upper_beats_left")]),
    "backward pass skipped": ("plane_refine", forward_only, [("refine", "staircase"), ("singles", "patches_15x15")]),
}
PLANE_RULES.update({"moments summed " + k: ("moment_total", v, [("far", "far")]) for k, v in other_orders().items()})


@pytest.mark.parametrize("rule", sorted(PLANE_RULES))
def test_a_changed_plane_rule_changes_the_result(rule):
    hook, value, scenes = PLANE_RULES[rule]
    for family, name in scenes:
        call = plane_calls(family)[name]
        base = plane_state(call)
        with changed(hook, value):
            assert plane_state(call) != base, (rule, family, name)


def across_boxes(call):
    """clusterObjects with edges allowed between the crops of different boxes of a cloud: components over all crops together, a
    box keeps its own points of the largest such component"""
    out = []
    crops = [PCC.crop(call.clouds[int(f)], b) for b, f in zip(call.boxes, call.frames)]
    for f in sorted(set(int(v) for v in call.frames)):
        mine = [i for i in range(len(call.boxes)) if int(call.frames[i]) == f]
        P = pc._xyz(call.clouds[f])
        allp = np.concatenate([P[crops[i]] for i in mine])
        lab = PCC.components(allp)
        size = np.bincount(lab, minlength=len(allp))
        pos = 0
        for i in mine:
            l = lab[pos:pos + len(crops[i])]
            pos += len(crops[i])
            if not len(l):
                out.append((i, ()))
                continue
            s = size[l]
            best = l[s == s.max()].min()
            out.append((i, tuple(int(v) for v in crops[i][l == best])))
    return tuple(v for _, v in sorted(out))


def less_one_direction(d):
    cells = pc.neighbour_cells()
    return lambda: [o for o in cells if o != d]


CLUSTER_RULES = {
    "a tie goes to the largest index": ("largest", lambda size: int(np.flatnonzero(size == size.max())[-1]),
                                        [("ties", "2x2"), ("ties", "3x2"), ("ties", "2x300"), ("ties", "3x300")]),
    "crop faces exclusive": ("inside", lambda p, lo, hi: (p > lo).all(axis=1) & (p < hi).all(axis=1), [("boxes", "on_faces")]),
}
CLUSTER_RULES.update({"26 neighbour cells: without %s and its opposite" % (d,): ("neighbour_cells", less_one_direction(d), [("faces", "faces")])
                      for d in pc.neighbour_cells() if d != (0, 0, 0)})


@pytest.mark.parametrize("rule", sorted(CLUSTER_RULES))
def test_a_changed_cluster_rule_changes_the_result(rule):
    hook, value, scenes = CLUSTER_RULES[rule]
    for family, name in scenes:
        call = cluster_calls(family)[name]
        base = cluster_state(call)
        with changed(hook, value):
            assert cluster_state(call) != base, (rule, family, name)


def test_every_direction_of_the_27_cells_decides_a_pair_of_faces():
    """without one of the 13 direction pairs, exactly the joined pairs across that direction and its opposite fall apart"""
    call = cluster_calls("faces")["faces"]
    base = [len(i) for i in cluster_reference("faces", "faces")[1]]
    for d in pc.neighbour_cells()[:-1]:
        with changed("neighbour_cells", less_one_direction(d)):
            got = [len(i) for i in PCC.clusterObjects(call.clouds, call.boxes, call.frames)[1]]
        lost = [k for k in range(len(base)) if got[k] != base[k]]
        dirs = {S.DIRECTIONS[(k // 4) % 26] for k in lost}
        assert dirs == {d, tuple(-v for v in d)} and len(lost) == 8, (d, lost)


def test_edges_across_boxes_change_the_result():
    call = cluster_calls("boxes")["300"]
    base = tuple(tuple(int(v) for v in i) for i in cluster_reference("boxes", "300")[1])
    assert across_boxes(call) != base
    alone = S.ClusterCall(call.clouds, call.boxes[:1], call.frames[:1])      # the restatement itself: one box, nothing to cross
    assert across_boxes(alone) == base[:1]


def test_radius_rule_cannot_change_a_result():
    """d2 <= r^2 against d2 < r^2: r^2 = (double)0.01f * (double)0.01f needs 46 mantissa bits, so no float32 d2 equals it (DESIGN.md
    section 6e, "Built hard clouds"); asserted here on the bits and on the scene with pairs an ulp either side of the radius"""
    r2 = float(pc.RADIUS) * float(pc.RADIUS)
    assert float(F(r2)) != r2
    assert pc.RADIUS2 == r2
    call = cluster_calls("faces")["faces"]
    base = cluster_state(call)
    with changed("within_radius", lambda d2: d2.astype(np.float64) < pc.RADIUS2):
        assert cluster_state(call) == base


def test_the_gpu_test_names_every_call_of_every_scene():
    G = _load("test_gpu_cloud_hard")
    assert {f: sorted(n) for f, n in G.PLANE_CALLS.items()} == {f: sorted(plane_calls(f)) for f in S.PLANE_SCENES}
    assert {f: sorted(n) for f, n in G.CLUSTER_CALLS.items()} == {f: sorted(cluster_calls(f)) for f in S.CLUSTER_SCENES if f != "crop_edge"}
