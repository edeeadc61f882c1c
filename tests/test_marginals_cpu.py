"""The max-marginal rule in numpy (partsbaseddetector_amd/marginals.py) against what it must mean: on dyadic inputs, whose sums
are all exact, an exhaustive float64 enumeration of every configuration; the root's marginals against the oracle's root scores bit
for bit; every part's largest marginal against the largest root score; the decoded poses against partscores.part_scores; and each
choice the rule makes shown to matter by flipping it.  No GPU."""
import numpy as np
import pytest

import marginal_cases as MC
from partsbaseddetector_amd import marginals as MG
from partsbaseddetector_amd import partscores as PS

DTYPES = ("float32", "float64")


def brute_force(flat, c, resp):
    """mm (NJ, H, W) float64 by enumeration: the score of every configuration, scattered by maximum to each part's (type, cell)"""
    _, H, W = resp.shape
    p0 = int(flat.part_offset[c])
    n = int(flat.part_offset[c + 1]) - p0
    ys, xs = np.mgrid[0:H, 0:W]
    ys, xs = ys.ravel(), xs.ravel()
    K = [len(MC.part_planes(flat, c, p)) for p in range(n)]
    # state of part p = (type, cell); axis p of the score tensor
    total = np.zeros([K[p] * H * W for p in range(n)], np.float64)
    shape = lambda p: [K[p] * H * W if q == p else 1 for q in range(n)]
    g0 = int(flat.mix_offset[p0])
    total += float(np.float32(flat.biasw[int(flat.biasid[g0])]))
    for p in range(n):
        gm0 = MC.part_planes(flat, c, p)[0]
        unary = np.concatenate([resp[int(flat.filterid[gm0 + m])].astype(np.float64).ravel() for m in range(K[p])])
        total = total + unary.reshape(shape(p))
        if p == 0:
            continue
        q = int(flat.parentid[p0 + p])
        pair = np.zeros((K[q] * H * W, K[p] * H * W), np.float64)
        for m in range(K[p]):
            d = int(flat.defid[gm0 + m])
            w = [float(np.float32(v)) for v in flat.defw[d]]
            dx = xs[:, None] + int(flat.anchors[d][0]) - xs[None, :]          # parent cell (rows) -> child cell (columns)
            dy = ys[:, None] + int(flat.anchors[d][1]) - ys[None, :]
            cost = -w[0] * dx * dx - w[1] * dx - w[2] * dy * dy - w[3] * dy
            for mq in range(K[q]):
                b = float(np.float32(flat.biasw[int(flat.biasid[gm0 + m]) + mq]))
                pair[mq * H * W:(mq + 1) * H * W, m * H * W:(m + 1) * H * W] = cost + b
        sh = [1] * n
        sh[q], sh[p] = pair.shape
        total = total + pair.reshape(sh)                   # q < p: the parent's axis comes first, as pair's rows
    mm = np.zeros((int(flat.mix_offset[-1]), H, W), np.float64)
    for p in range(n):
        best = total.max(axis=tuple(q for q in range(n) if q != p)).reshape(K[p], H, W)
        gm0 = MC.part_planes(flat, c, p)[0]
        mm[gm0:gm0 + K[p]] = best
    return mm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["chain", "star", "chain1"])
def test_dyadic_marginals_equal_the_exhaustive_maximum(name, dtype):
    flat = MC.model(name, "dyadic").flatten()
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (2, 3), (4, 5)):
        resp = rng.integers(-4, 5, (flat.nfilters, H, W)).astype(dtype)
        mm = MG.max_marginals(flat, 0, resp)[0]
        want = brute_force(flat, 0, resp)
        assert mm.dtype == np.dtype(dtype)
        assert np.array_equal(mm.astype(np.float64), want), (name, H, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,levels", MC.CASES)
def test_root_marginals_are_the_root_scores_and_every_part_reaches_the_best(name, levels, dtype, oracle):
    for values in MC.VALUES:
        flat = MC.model(name, values).flatten()
        resp = MC.responses(name, levels, values, dtype)
        for l, per_c in enumerate(MC.yardstick(name, levels, values, dtype)):
            for c, d in enumerate(per_c):
                rootv, rooti = oracle.dp_min(flat, c, resp[l])[3:]
                pl = MC.part_planes(flat, c, 0)
                v, i = MG.reduce_max([d["mm"][g] for g in pl])
                assert v.tobytes() == rootv.tobytes() and np.array_equal(i, rooti), (name, values, l, c)
                if values == "dyadic":                         # exact sums: every part's best marginal is the best root score
                    n = int(flat.part_offset[c + 1]) - int(flat.part_offset[c])
                    for p in range(n):
                        pp = MC.part_planes(flat, c, p)
                        assert d["mm"][pp[0]:pp[-1] + 1].max() == rootv.max(), (name, l, c, p)


MUTATIONS = [("sibling_order", "ascending", "star", "dense"), ("skip_self", False, "chain", "dyadic"),
             ("mirror_linear", False, "tree", "dyadic"), ("mirror_anchor", False, "tree", "dyadic"), ("first_wins", False, "star", "dyadic")]


@pytest.mark.parametrize("kw,value,name,values", MUTATIONS)
def test_each_choice_of_the_rule_changes_an_output(kw, value, name, values):
    flat = MC.model(name, values).flatten()
    changed = False
    for l, resp in enumerate(MC.responses(name, "A", values, "float32")):
        got = MG.max_marginals(flat, 0, resp, **{kw: value})
        want = MC.yardstick(name, "A", values, "float32")[l][0]
        changed = changed or any(g.tobytes() != want[k].tobytes() for g, k in zip(got, ("mm", "down", "Jx", "Jy", "Jk")))
    assert changed, kw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["chain", "star", "tree", "two", "slices"])
def test_decoded_poses_score_what_their_seed_promised(name, dtype):
    """dyadic values: the pose decoded from a seed, scored part by part (partscores.part_scores), adds up to the seed's
    max-marginal exactly, and holds the seed's part at the seed's cell"""
    flat = MC.model(name, "dyadic").flatten()
    seeds = MC.seeds_of(name, "A", "dyadic", dtype)
    status, rec, place = MC.decode_all(name, "A", "dyadic", dtype, seeds)
    resp = MC.responses(name, "A", "dyadic", dtype)
    ys = MC.yardstick(name, "A", "dyadic", dtype)
    assert (status > 0).sum() >= 6 and (status == -1).sum() == 9
    for i, s in enumerate(seeds):
        if status[i] < 0:
            continue
        l, c, p, t, x, y = (int(v) for v in s)
        k = int(status[i])
        pl = [tuple(int(v) for v in q) for q in place[i, :k]]
        assert pl[p][:2] == (x, y) and (t < 0 or pl[p][2] == t)
        sc = PS.part_scores(flat, resp[l], c, pl, np.dtype(dtype))
        want = ys[l][c]["mm"][MC.part_planes(flat, c, p)[0] + pl[p][2], y, x]
        assert sc[0, PS.MESSAGE] == want, (name, i, s)
        assert rec[i, 5:6].view(np.float32)[0] == np.float32(want) and rec[i, 6] == k and tuple(rec[i, 3:5]) == pl[0][:2]
