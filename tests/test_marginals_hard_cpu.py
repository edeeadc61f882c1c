"""The hard cases of the max-marginal tests (tests/marginal_cases.py: the wide models, the non-finite response sets), checked on the
CPU before tests/test_gpu_marginals_hard.py compares the kernels with them.  No GPU.

* The wide models on dyadic values equal the exhaustive maximum on levels small enough to enumerate, and satisfy the root identity
  on their level sets; "wide16" does record parent types of index 8 and above, does hold ties between parent types of index 4 and
  above and of index 8 and above in which the lower index is recorded, and every choice of the rule changes one of its outputs.
* Every non-finite case: the oracle's NaN intersections, counted apart over the upward and the mirrored transforms.  Where none
  forms under either read-out, "reference" and "max" give the same bytes.  For every model, neg_region and nan_cells form some in
  the mirrored transforms and the two read-outs differ in down, Jx and Jy there: a kernel that followed the reference's loop would
  be told apart.  (pos_spikes, class F for the upward pass, floods "tree" and "wide16" with +Inf: their mirrored transforms push
  NaN intersections, and as for pos_pair no read-out can tell the rules apart on them.)
* The root identity under "max": reduceMax over the root's mm planes is the oracle's rootv of dp_min(readout="max").
* Type -1 seeds on a cell where every mm of the part is NaN, and on one where every mm is -Inf, decode to type 0.
* The mirrored context planes reach the distance transform's hard paths: replayed (dt_hard_planes.replay_dt, rule "max") with their
  mirrored quadratics, some context plane of the "i16" set has rows and columns deeper than the deepest ring (512 entries), a NaN
  entry among the spilled, and some of the "u8" set pops a whole cooperative window of 16 for one element, in both passes; for
  every forced launch setting every form it runs is reached."""
import functools

import numpy as np
import pytest

import dt_hard_planes as H
import marginal_cases as MC
from partsbaseddetector_amd import marginals as MG
from test_gpu_dt_planes import SETTINGS, _paths
from test_marginals_cpu import brute_force

DTYPES = ("float32", "float64")
KEYS = ("mm", "down", "Jx", "Jy", "Jk")


# ---- the wide models -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["wide8", "wide16"])
def test_wide_dyadic_marginals_equal_the_exhaustive_maximum(name, dtype):
    flat = MC.model(name, "dyadic").flatten()
    rng = np.random.default_rng(5)
    for Hh, W in ((1, 1), (1, 3), (2, 2)):
        resp = rng.integers(-4, 5, (flat.nfilters, Hh, W)).astype(dtype)
        mm = MG.max_marginals(flat, 0, resp)[0]
        assert mm.dtype == np.dtype(dtype)
        assert np.array_equal(mm.astype(np.float64), brute_force(flat, 0, resp)), (name, Hh, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,levels", MC.WIDE_CASES)
def test_wide_root_marginals_are_the_root_scores_and_every_part_reaches_the_best(name, levels, dtype, oracle):
    for values in MC.VALUES:
        flat = MC.model(name, values).flatten()
        resp = MC.responses(name, levels, values, dtype)
        for l, per_c in enumerate(MC.yardstick(name, levels, values, dtype)):
            d = per_c[0]
            rootv, rooti = oracle.dp_min(flat, 0, resp[l])[3:]
            v, i = MG.reduce_max([d["mm"][g] for g in MC.part_planes(flat, 0, 0)])
            assert v.tobytes() == rootv.tobytes() and np.array_equal(i, rooti), (name, values, l)
            if values == "dyadic":
                for p in range(int(flat.part_offset[1])):
                    pp = MC.part_planes(flat, 0, p)
                    assert d["mm"][pp[0]:pp[-1] + 1].max() == rootv.max(), (name, l, p)


def _parent_type_ties(name, levels):
    """over every non-root plane of the dyadic yardstick: cells whose recorded parent type is >= 8; cells where the maximum is
    attained by a second parent type above the recorded one (the rule run with the last of equals winning records a higher index),
    the recorded one being >= 4, and >= 8"""
    flat = MC.model(name, "dyadic").flatten()
    high = tie4 = tie8 = 0
    for l, resp in enumerate(MC.responses(name, levels, "dyadic", "float32")):
        first = MC.yardstick(name, levels, "dyadic", "float32")[l][0]["Jk"]
        last = MG.max_marginals(flat, 0, resp, first_wins=False)[4]
        for p in range(1, int(flat.part_offset[1])):
            for g in MC.part_planes(flat, 0, p):
                a, b = first[g], last[g]
                high += int((a >= 8).sum())
                tie4 += int(((a >= 4) & (b > a)).sum())
                tie8 += int(((a >= 8) & (b > a)).sum())
    return high, tie4, tie8


def test_wide_models_hold_high_parent_types_and_ties_among_them():
    high, tie4, tie8 = _parent_type_ties("wide16", "B")
    assert high > 100 and tie4 > 10 and tie8 > 10, (high, tie4, tie8)
    _, tie4, _ = _parent_type_ties("wide8", "A")
    assert tie4 > 10, tie4


MUTATIONS = [("sibling_order", "ascending", "dense"), ("skip_self", False, "dyadic"), ("mirror_linear", False, "dyadic"),
             ("mirror_anchor", False, "dyadic"), ("first_wins", False, "dyadic")]


@pytest.mark.parametrize("kw,value,values", MUTATIONS)
def test_each_choice_of_the_rule_changes_an_output_of_wide16(kw, value, values):
    flat = MC.model("wide16", values).flatten()
    changed = False
    for l, resp in enumerate(MC.responses("wide16", "A", values, "float32")):
        got = MG.max_marginals(flat, 0, resp, **{kw: value})
        want = MC.yardstick("wide16", "A", values, "float32")[l][0]
        changed = changed or any(g.tobytes() != want[k].tobytes() for g, k in zip(got, KEYS))
    assert changed, kw


# ---- the non-finite cases ------------------------------------------------------------------------------------------------------
def _differing(a, b, key):
    """cells of plane block `key` in which two yardsticks differ, NaN equal to NaN"""
    n = 0
    for la, lb in zip(a, b):
        x, y = la[0][key], lb[0][key]
        same = (x == y) | (np.isnan(x) & np.isnan(y)) if x.dtype.kind == "f" else x == y
        n += int((~same).sum())
    return n


# kinds whose mirrored transforms push NaN intersections, per model, as measured (the test asserts the table): the one +Inf cell
# of pos_spikes, in the filters of the root's children, leaves the chain "slices" without any, and turns the context planes of
# "tree" and "wide16", whose roots have several children, into +Inf
MIRRORED_NAN = {"tree": {"pos_spikes", "neg_region", "pos_pair", "nan_cells"}, "slices": {"neg_region", "pos_pair", "nan_cells"},
                "wide16": {"pos_spikes", "neg_region", "pos_pair", "nan_cells"}}


@pytest.mark.parametrize("set_name", MC.NF_SETS)
@pytest.mark.parametrize("kind", MC.NF_KINDS)
@pytest.mark.parametrize("name", [m for m, _ in MC.NF_MODELS])
def test_nonfinite_counts_and_read_outs(name, kind, set_name):
    for dtype in DTYPES:
        mx, n_mx = MC.nf_yardstick(name, kind, set_name, dtype)
        ref, n_ref = MC.nf_yardstick(name, kind, set_name, dtype, "reference")
        print(f"NaN intersections {name} {kind} {set_name} {dtype}: max upward {n_mx['upward']} mirrored {n_mx['mirrored']}; "
              f"reference upward {n_ref['upward']} mirrored {n_ref['mirrored']}")
        assert (n_mx["mirrored"] > 0) == (kind in MIRRORED_NAN[name]), n_mx
        if kind in H.NONFINITE_F:
            assert n_mx["upward"] == 0 and n_ref["upward"] == 0          # class F is a statement about the upward pass
        if sum(n_mx.values()) + sum(n_ref.values()) == 0:
            for key in KEYS + ("IxRaw", "IyRaw", "Ik", "rootv", "rooti"):
                assert all(a[0][key].tobytes() == b[0][key].tobytes() for a, b in zip(mx, ref)), key
        if kind in ("neg_region", "nan_cells"):
            assert n_mx["mirrored"] > 0
            for key in ("down", "Jx", "Jy"):
                assert _differing(mx, ref, key) > 0, key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [m for m, _ in MC.NF_MODELS])
def test_nonfinite_root_marginals_are_the_oracles_root_scores(name, dtype, oracle):
    """the identity that ties the yardstick to the oracle's dynamic program holds under "max" on every kind: NaN at the same
    places, the same bits elsewhere, the same type wherever the score is no NaN"""
    flat = MC.model(name, MC.nf_values(name)).flatten()
    for kind in MC.NF_KINDS:
        resp = MC.nf_responses(name, kind, "u8", dtype)
        for l, per_c in enumerate(MC.nf_yardstick(name, kind, "u8", dtype)[0]):
            rootv, rooti = oracle.dp_min(flat, 0, resp[l], readout="max")[3:]
            v, i = MG.reduce_max([per_c[0]["mm"][g] for g in MC.part_planes(flat, 0, 0)])
            assert np.array_equal(v, rootv, equal_nan=True) and np.array_equal(i, rooti), (kind, l)
            assert np.array_equal(per_c[0]["rootv"], rootv, equal_nan=True) and np.array_equal(per_c[0]["rooti"], rooti), (kind, l)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [m for m, _ in MC.NF_MODELS])
def test_seeds_on_all_nan_and_all_neginf_cells_decode_to_type_0(name, dtype):
    flat = MC.model(name, MC.nf_values(name)).flatten()
    cells = MC.nf_cells(name, "nan_cells", "u8", dtype)
    assert len(cells["nan"]) >= 1 and len(cells["neginf"]) >= 1 and len(cells["finite"]) == int(flat.part_offset[1])
    ys = MC.nf_yardstick(name, "nan_cells", "u8", dtype)[0]
    seeds = MC.nf_seeds(name, "nan_cells", "u8", dtype)
    status, rec, place = MC.decode_seeds(flat, ys, MC.nf_shapes("u8"), MC.nf_scales("u8"), dtype, seeds)
    assert (status == -1).sum() == 9
    several = False
    for key, test in (("nan", np.isnan), ("neginf", np.isneginf)):
        for s in cells[key]:
            l, _, p, t, x, y = s
            i = int(np.flatnonzero((seeds == np.asarray(s, np.int32)).all(1))[0])
            pl = MC.part_planes(flat, 0, p)
            assert t == -1 and test(ys[l][0]["mm"][pl[0]:pl[-1] + 1, y, x]).all()
            assert status[i] == int(flat.part_offset[1]) and tuple(place[i, p]) == (x, y, 0), (key, s)
            assert test(rec[i, 5:6].view(np.float32))[0], (key, s)           # the score is the mm of type 0: NaN, or -Inf
            several = several or len(pl) > 1
    assert several                                                           # not only one-type parts, which copy


def _mirrored_quadratic(flat, p):
    """(a_x, b_x, a_y, b_y, os_x, os_y) of the mirrored transform of part p's type 0"""
    d = int(flat.defid[int(flat.mix_offset[p])])
    w = [float(v) for v in flat.defw[d]]
    return -w[0], w[1], -w[2], w[3], -int(flat.anchors[d][0]), -int(flat.anchors[d][1])


@functools.lru_cache(maxsize=None)
def _context_stats(dtype):
    """(set, pass) -> over every context plane C_p[mq] of "slices" under every kind, replayed with the mirrored quadratic of type 0:
    the deepest envelope, the most entries popped for one element, and over the lines with a NaN intersection the most entries
    between the top and the lowest NaN entry"""
    flat = MC.model("slices", MC.nf_values("slices")).flatten()
    stats = {}
    for set_name in MC.NF_SETS:
        for kind in MC.NF_KINDS:
            for resp in MC.nf_responses("slices", kind, set_name, dtype):
                ctx = {}
                MG.max_marginals(flat, 0, resp, readout="max", contexts=ctx)
                for (p, _), plane in ctx.items():
                    _, st_r, st_c = H.replay_dt(plane, *_mirrored_quadratic(flat, p), np.dtype(dtype).type, readout="max")
                    for pas, st in (("rows", st_r), ("cols", st_c)):
                        d, pops, nd = stats.get((set_name, pas), (0, 0, 0))
                        n = st["nan_isect"] > 0
                        below = int((st["top"] + 1 - st["nan_floor"])[n].max()) if n.any() else 0
                        stats[set_name, pas] = (max(d, int(st["depth"].max())), max(pops, int(st["maxpop"].max())), max(nd, below))
    return stats


@pytest.mark.parametrize("handle", ["f32", "f64"])
def test_mirrored_context_planes_reach_the_paths(handle):
    stats = _context_stats("float64" if handle == "f64" else "float32")
    for pas in ("rows", "cols"):
        depth, _, nan_depth = stats["i16", pas]
        assert depth >= 512 + 2 and nan_depth >= 512 + 2, (pas, stats)       # the deepest ring spills, a NaN entry among the spilled
        assert stats["u8", pas][1] >= 16, (pas, stats)                       # a whole cooperative window popped for one element
    for setting, options in SETTINGS.items():
        if not options:
            continue
        reached = {}
        for set_name in MC.NF_SETS:
            for pas, (form, size) in _paths(handle, options, set_name).items():
                d, p, _ = stats[set_name, pas]
                got = d >= size + 2 if form == "ring" else p >= size         # a ring of T spills once T + 2 entries are live
                reached[form, size] = reached.get((form, size), False) or got
        assert all(reached.values()), (setting, reached, stats)
