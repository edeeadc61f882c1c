"""The part-score rule of partsbaseddetector_amd/partscores.py on the CPU, against the dynamic program
restated in numpy over the oracle's distance transform (partscores.accumulated) and against oracle.dp_min.

Arg-max walk: the root value the rule rebuilds from the placement has the bits of the record's score, and every part's total is
the plane the dynamic program had accumulated for it, for every record of every model whose inner parts own their filter ids.
Reference walk: never above the score, below it for some record.  The tree whose inner parts share filter ids keeps neither
equality, and the test says so, so that the documented limit stays true.  Each choice the rule makes (child order, one rounding
per pass, the root's bias) is shown to matter by a mutation that changes a value.  No GPU."""
import functools

import numpy as np
import pytest

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import partscores as PS
from partsbaseddetector_amd import synth

TREE_PA = [0, 1, 2, 2, 1, 5, 5, 3]      # 8 parts, depth 3; parts 1, 2 and 4 have children, 1 and 4 two each
PER_PLANE = 12                          # records sampled per (level, component)


def tree_model(inner_shared=False):
    m = M.synthetic_model(seed=7, pa=TREE_PA, nmix=3, linear_def=True, interval=5, thresh=-100.0)
    if inner_shared:
        m.filterid[0][4] = list(m.filterid[0][1])   # two parts that both have children
        m.validate()
    return m


def shared_leaf_model():
    m = M.synthetic_tiny_model(thresh=-1.0)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def root_bias_model():
    """the tiny model with a bias of its own for every root mixture (the synthetic builders give the root one)"""
    m = M.synthetic_tiny_model(thresh=-1.0)
    ids = [m.biasid[0][0][0]]
    for k in range(1, len(m.filterid[0][0])):
        ids.append(len(m.biasw))
        m.biasw.append(0.25 * k)
    m.biasid[0][0] = ids
    m.validate()
    return m


CASES = {
    "tiny": (lambda: M.synthetic_tiny_model(thresh=-1.0), 5, 72, 96),
    "tiny_quadratic": (lambda: M.synthetic_tiny_model(thresh=-1.0, linear_def=False), 5, 72, 96),
    "shared_leaf": (shared_leaf_model, 5, 72, 96),
    "face": (lambda: M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0), 3, 64, 80),
    "tree": (tree_model, 3, 64, 80),
    "tree_inner_shared": (lambda: tree_model(True), 3, 64, 80),
    "root_bias": (root_bias_model, 5, 72, 96),
}


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(flat, [per sampled record: level, c, x, y, resp, maps of partscores.accumulated, maps of oracle.dp_min])"""
    from oracle import oracle
    make, seed, rows, cols = CASES[name]
    flat = make().flatten()
    feats, _ = oracle.features_pyramid(flat, synth.synthetic_frame(seed, rows, cols), dtype)
    rng = np.random.default_rng(11)
    out = []
    for lvl, feat in enumerate(feats):
        resp = oracle.responses(flat, feat)
        for c in range(flat.ncomponents):
            acc = PS.accumulated(flat, c, resp)
            ref = oracle.dp_min(flat, c, resp)
            ys, xs = np.nonzero(acc[3] > dtype(flat.thresh))
            for k in rng.permutation(len(ys))[:PER_PLANE]:
                out.append((lvl, c, int(xs[k]), int(ys[k]), resp, acc, ref))
    assert len(out) >= 40, (name, len(out))
    return flat, out


def bits(v):
    return np.float32(v).view(np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["tiny", "tiny_quadratic", "shared_leaf", "face", "tree", "root_bias"])
def test_argmax_walk_rebuilds_the_score_and_the_accumulated_planes(name, dtype):
    flat, recs = case(name, dtype)
    for lvl, c, x, y, resp, (IxRaw, IyRaw, Ik, rootv, rooti, planes), _ in recs:
        pl = E.walk(flat, c, x, y, IxRaw, IyRaw, Ik, rooti, argmax=True)
        s = PS.part_scores(flat, resp, c, pl, dtype)
        assert s.dtype == dtype
        assert bits(s[0, PS.MESSAGE]) == bits(rootv[y, x]), (lvl, c, x, y)
        for p, (px, py, m) in enumerate(pl):
            assert s[p, PS.TOTAL].tobytes() == planes[p][m][py, px].tobytes(), (lvl, c, x, y, p)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["tiny", "tiny_quadratic", "face", "tree", "tree_inner_shared"])
def test_reference_walk_is_never_above_and_somewhere_below(name, dtype):
    flat, recs = case(name, dtype)
    below = 0
    for lvl, c, x, y, resp, _, (Ix, Iy, Ik, rootv, rooti) in recs:
        pl = E.walk(flat, c, x, y, Ix, Iy, Ik, rooti)
        got = np.float32(PS.part_scores(flat, resp, c, pl, dtype)[0, PS.MESSAGE])
        score = np.float32(rootv[y, x])
        assert got <= score, (lvl, c, x, y, got, score)
        below += got < score
    assert below >= 1


def test_inner_shared_filter_ids_keep_no_identity():
    """the reference keys its accumulators by filter id: a plane two inner parts share holds both parts' messages, which no
    placement's own sum contains"""
    flat, recs = case("tree_inner_shared", np.float32)
    equal = 0
    for lvl, c, x, y, resp, (IxRaw, IyRaw, Ik, rootv, rooti, _), _ in recs:
        pl = E.walk(flat, c, x, y, IxRaw, IyRaw, Ik, rooti, argmax=True)
        equal += bits(PS.part_scores(flat, resp, c, pl, np.float32)[0, PS.MESSAGE]) == bits(rootv[y, x])
    assert equal == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["tiny", "tree"])
def test_root_message_agrees_with_the_float64_placement_score(name, dtype):
    """Every part adds at most four roundings of a partial sum (two passes, two adds), each at most u times the sum of the
    magnitudes of the terms so far: (4 nparts + 8) u sum|terms|, in the manner of examples.rounding_bound."""
    flat, recs = case(name, dtype)
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    for lvl, c, x, y, resp, _, (Ix, Iy, Ik, rootv, rooti) in recs:
        pl = E.walk(flat, c, x, y, Ix, Iy, Ik, rooti)
        s = PS.part_scores(flat, resp, c, pl, dtype).astype(np.float64)
        want = E.placement_score(flat, resp, c, pl)
        mag = np.abs(s[:, PS.APPEARANCE]).sum() + np.abs(s[:, PS.BIAS]).sum() + np.abs(s[1:, PS.MESSAGE] - s[1:, PS.TOTAL]).sum()
        assert abs(s[0, PS.MESSAGE] - want) <= (4 * len(pl) + 8) * u * mag, (lvl, c, x, y)


def changed(name, dtype, **mutation):
    flat, recs = case(name, dtype)
    n = 0
    for lvl, c, x, y, resp, (IxRaw, IyRaw, Ik, rootv, rooti, _), _ in recs:
        pl = E.walk(flat, c, x, y, IxRaw, IyRaw, Ik, rooti, argmax=True)
        n += PS.part_scores(flat, resp, c, pl, dtype).tobytes() != PS.part_scores(flat, resp, c, pl, dtype, **mutation).tobytes()
    return n


def test_each_choice_of_the_rule_changes_a_value():
    # a parent with two children: the order of its two adds
    assert changed("tree", np.float32, child_order="ascending") > 0
    # one rounding for both passes instead of one per pass
    assert changed("tiny", np.float32, passes="one") > 0
    # the root's bias: the synthetic builders give the root ONE bias (mixtures past 0 have none), so the model is built
    flat, _ = case("root_bias", np.float32)
    g0 = int(flat.mix_offset[flat.part_offset[0]])
    rb = [float(flat.biasw[int(flat.biasid[g0 + k])]) for k in range(int(flat.mix_offset[flat.part_offset[0] + 1]) - g0)]
    assert len(set(rb)) == len(rb) > 1
    assert changed("root_bias", np.float32, root_bias="winning") > 0


def test_scores_of_records_marks_bad_placements():
    flat, recs = case("tiny", np.float32)
    lvl, c, x, y, resp, _, (Ix, Iy, Ik, rootv, rooti) = recs[0]
    pl = np.asarray(E.walk(flat, c, x, y, Ix, Iy, Ik, rooti), np.int32)
    H, W = resp.shape[1:]
    assert PS.placement_valid(flat, c, [tuple(q) for q in pl], H, W)
    for q, k, v in ((1, 0, W), (2, 1, -1), (0, 2, 2), (1, 2, -1)):
        bad = pl.copy()
        bad[q, k] = v
        assert not PS.placement_valid(flat, c, [tuple(r) for r in bad], H, W)


def test_new_symbols_are_exported():
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = _lib.load()
    for n in ("pbd_part_scores", "pbd_part_scores_device", "pbd_score_placements", "pbd_score_placements_device"):
        assert hasattr(lib, n), n
