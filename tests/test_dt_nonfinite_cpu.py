"""The yardsticks of tests/test_gpu_dt_nonfinite.py, checked on the CPU: the oracle's two read-out rules for the distance transform
("reference": computeRow's own loop; "max": entry max{k : z[k] < os + q} with comparisons against NaN false -- include/pbd.h,
pbd_dp_min, "Non-finite scores"), the replay of computeRow in tests/dt_hard_planes.py under both rules, and the planes with
infinite and NaN scores.

* Where the reference is well defined -- every hard plane the suite already has, every class F plane -- no NaN intersection forms
  and the two rules give the same bytes: rule "max" changes nothing there.
* On class N planes the rules select different entries, so a kernel that follows the wrong one is caught.  (Not on pos_pair:
  test_pos_pair_rules_coincide says why.)
* replay_rows, which looks at every entry of the finished envelope for "max", and the oracle, which walks down from the top, are
  two statements of each rule; they must agree on the leaf transforms of both classes.
* Class F against brute force: the output is the maximum over source cells of quadratic + score, the pointer attains it, a -Inf
  cell is never chosen and a +Inf cell always."""
import numpy as np
import pytest

import dp_hard_models as DP
import dt_hard_planes as H
import dt_wave_replay as W
import test_gpu_dt_nonfinite as G
import test_gpu_dt_planes as P


def _dp_both(oracle, flat, s):
    """dp_min of every component under both rules, and the NaN intersections of both runs together."""
    ref, mx, nans = [], [], 0
    for c in range(flat.ncomponents):
        ref.append(oracle.dp_min(flat, c, s))
        nans += oracle.nan_isect()
        mx.append(oracle.dp_min(flat, c, s, readout="max"))
        nans += oracle.nan_isect()      # (the columns pass scans what the rows pass read out: the counts may differ)
    return ref, mx, nans


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _existing_hard_inputs():
    """(id, flat, planes per level) of every built-input set the dynamic program's GPU tests use."""
    for tree, deformation in P.MODELS:
        flat = H.dt_model(tree, deformation).flatten()
        for set_name in P.SETS:
            for handle in P.HANDLES:
                yield f"dt-{tree}-{deformation}-{set_name}-{handle}", flat, P._inputs(handle, flat, set_name)[1]
    for name, model in (("ragged", DP.ragged_model()), ("table3", DP.table_model(3)), ("table8", DP.table_model(8))):
        for set_name, dims in DP.SETS.items():
            yield f"dp-{name}-{set_name}", model.flatten(), DP.quantised_scores(model, dims, DP.RAGGED_SEED)


def test_rules_agree_on_every_existing_hard_plane(oracle):
    n = 0
    for ident, flat, planes in _existing_hard_inputs():
        for l, s in enumerate(planes):
            ref, mx, nans = _dp_both(oracle, flat, s)
            assert nans == 0, (ident, l)
            assert all(_same_bytes(r, m) for r, m in zip(ref, mx)), (ident, l)
            n += 1
    assert n > 300


@pytest.mark.parametrize("handle,kind", [(h, k) for h in G.HANDLES for k in H.NONFINITE_F if G._applies(h, k)])
def test_rules_agree_on_class_f(oracle, handle, kind):
    for tree, deformation in G.MODELS:
        flat = G._flat(tree, deformation)
        for set_name in G.LEVELS:
            for l, s in enumerate(G._inputs(handle, tree, deformation, kind, set_name)[1]):
                ref, mx, nans = _dp_both(oracle, flat, s)
                assert nans == 0, (tree, deformation, set_name, l)
                assert all(_same_bytes(r, m) for r, m in zip(ref, mx)), (tree, deformation, set_name, l)


@pytest.mark.parametrize("kind", ["neg_region", "nan_cells"])
@pytest.mark.parametrize("handle", G.HANDLES)
def test_rules_differ_on_class_n(oracle, handle, kind):
    """On every class N plane of more than four cells a NaN intersection forms and the two rules differ in a pointer."""
    for tree, deformation in G.MODELS:
        flat = G._flat(tree, deformation)
        for set_name in G.LEVELS:
            for l, s in enumerate(G._inputs(handle, tree, deformation, kind, set_name)[1]):
                if s[0].size <= 4:
                    continue
                ref, mx, nans = _dp_both(oracle, flat, s)
                assert nans > 0, (tree, deformation, set_name, l)
                differ = sum(int((r[0] != m[0]).sum() + (r[1] != m[1]).sum()) for r, m in zip(ref, mx))
                assert differ > 0, (tree, deformation, set_name, l)


@pytest.mark.parametrize("handle", G.HANDLES)
def test_pos_pair_rules_coincide(oracle, handle):
    """Two neighbouring +Inf do push a NaN intersection (Inf - Inf), yet no read-out can tell the rules apart on them: the first
    +Inf pops the whole envelope (its intersection with every finite entry is -Inf), the second is pushed with z = NaN, and every
    entry pushed above a +Inf entry gets z = +Inf (a finite or -Inf score) or NaN (another +Inf), neither of which is below any
    os + q.  So the walk up stops under the NaN and the walk down passes the same entries: both end on the first +Inf (a binary
    search of that z[] ends there too).  The kind stays in the GPU test as a class N member -- NaN in the scan, in the ring's
    spilled records, in the combine and root sums -- and this test pins the reason it separates no two read-outs."""
    total = 0
    for tree, deformation in G.MODELS:
        flat = G._flat(tree, deformation)
        for set_name in G.LEVELS:
            for l, s in enumerate(G._inputs(handle, tree, deformation, "pos_pair", set_name)[1]):
                ref, mx, nans = _dp_both(oracle, flat, s)
                total += nans
                assert all(_same_bytes(r[:3], m[:3]) for r, m in zip(ref, mx)), (tree, deformation, set_name, l)
    assert total > 0


def _real_bits(a):
    """bytes of a real array with every NaN made the same one"""
    a = a.copy()
    a[np.isnan(a)] = np.nan
    return a.tobytes()


@pytest.mark.parametrize("readout", ["reference", "max"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_replay_equals_the_oracles_leaf_transforms(oracle, kind, readout):
    """Values, both pointer planes (Iy composed as the reference does, IyRaw[m][Ix[m][n]]) and the count of NaN intersections."""
    handle = "f16" if kind == "f16_sat" else "f32"
    differ = 0
    for tree, deformation in G.MODELS:
        flat = G._flat(tree, deformation)
        jobs = H.leaf_jobs(flat)[::2]
        for set_name in G.LEVELS:
            for l, s in enumerate(G._inputs(handle, tree, deformation, kind, set_name)[1]):
                for f, ax, bx, ay, by, osx, osy in jobs:
                    out, Ix, Iy = oracle.dt(s[f], ax, bx, ay, by, osx, osy, readout=readout)
                    nans = oracle.nan_isect()
                    tmp, px, st_r = H.replay_rows(s[f], ax, bx, osx, readout=readout)
                    got, py, st_c = H.replay_rows(tmp.T, ay, by, osy, readout=readout)
                    where = (tree, deformation, set_name, l, f)
                    assert _real_bits(got.T) == _real_bits(out), where
                    assert np.array_equal(px, Ix), where
                    assert np.array_equal(np.take_along_axis(py.T, px, axis=1), Iy), where
                    assert nans == int(st_r["nan_isect"].sum() + st_c["nan_isect"].sum()), where
                    if readout == "max" and kind in ("neg_region", "nan_cells"):
                        _, rx, _ = H.replay_rows(s[f], ax, bx, osx)
                        differ += int((rx != px).sum())
    if readout == "max" and kind in ("neg_region", "nan_cells"):
        assert differ > 0       # the replay's two rules are two rules


BRUTE = [((9, 40), (0.25, 0.0, 0.015625, 0.0), (0, 0)), ((33, 17), (0.015625, 0.5, 0.25, 0.0), (3, -2)),
         ((3, 300), (0.0625, -0.25, 0.0625, 0.125), (-4, 1)), ((70, 2), (0.25, 0.0, 0.0625, -0.5), (1, 4)),
         ((1, 65), (0.015625, 0.0, 0.015625, 0.0), (2, 0)), ((2, 2), (0.25, 0.5, 0.0625, 0.0), (0, 1))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", H.NONFINITE_F)
@pytest.mark.parametrize("shape,w,os", BRUTE)
def test_class_f_against_brute_force(oracle, kind, shape, w, os, dtype):
    """Quantised planes (multiples of 1/4) with the class F cells and power-of-two coefficients: every finite intermediate value
    is exact, so, as in test_oracle_cpu.py::test_dt_exact_on_hard_planes, the transform equals the O(N^2) maximum in float64 bit
    for bit and each pointer attains it; a -Inf cell is never pointed at, and the one +Inf cell is by every cell of its row
    (then, in the columns pass, its row by every cell).  Both rules."""
    rng = np.random.default_rng(len(kind) * 11 + shape[1])
    score = H.nonfinite_plane(kind, rng, *shape, base="quantised")
    if kind == "f16_sat":
        with np.errstate(over="ignore"):
            score = score.astype(np.float16)
    score = score.astype(dtype)
    assert np.isinf(score).any() and not np.isnan(score).any()
    ax, bx, ay, by = (-float(np.float32(v)) for v in w)
    M_, N_ = shape
    s64 = score.astype(np.float64)
    dx = (os[0] + np.arange(N_)[:, None] - np.arange(N_)[None, :]).astype(np.float64)         # [out n, source n']
    row_max = ((ax * dx * dx + bx * dx)[None, :, :] + s64[:, None, :]).max(axis=2)
    dy = (os[1] + np.arange(M_)[:, None] - np.arange(M_)[None, :]).astype(np.float64)         # [out m, source m']
    ref = ((ay * dy * dy + by * dy)[:, :, None] + row_max[None, :, :]).max(axis=1)
    m, n = np.mgrid[0:M_, 0:N_]
    for readout in ("reference", "max"):
        out, Ix, Iy = oracle.dt(score, ax, bx, ay, by, os[0], os[1], readout=readout)
        assert oracle.nan_isect() == 0
        assert np.array_equal(out, ref.astype(dtype)), readout
        ddx = (os[0] + n - Ix).astype(np.float64)
        assert np.array_equal(ax * ddx * ddx + bx * ddx + s64[m, Ix], row_max), readout      # the row pointer is an arg-max
        ddy = (os[1] + m - Iy).astype(np.float64)
        assert np.array_equal(ay * ddy * ddy + by * ddy + row_max[Iy, Ix], ref[m, Ix]), readout
        assert not np.isneginf(s64[m, Ix]).any(), readout
        spiked = np.isposinf(s64).any(axis=1)
        assert np.isposinf(s64[m, Ix])[spiked].all() and (not spiked.any() or np.isposinf(out).all()), readout


@pytest.mark.parametrize("kind", ["neg_region", "nan_cells", "pos_pair"])
def test_wave_replay_follows_the_max_readout(kind):
    """The CPU replay of one streamed wave (ring, spills, whole-wave service: tests/dt_wave_replay.py) walks down from the top as
    dt_stream does; its own line-by-line comparison with plain_rows (rule "max") holds on class N rows, and plain_rows equals
    replay_rows(readout="max")."""
    rng = np.random.default_rng(5)
    planes = [H.nonfinite_plane(kind, rng, h, w, base=base) for h, w, base in [(17, 128, "constant"), (16, 65, "spikes"), (70, 40, "quantised")]]
    outs, counts = W.replay_levels(planes, -0.01, -0.0, 1)
    assert counts["spill_paths"] > 0 and counts["service_ro"] + counts["fallback_ro"] > 0
    for p, o in zip(planes, outs):
        want, _, st = H.replay_rows(p, -0.01, -0.0, 1, readout="max")
        assert st["nan_isect"].sum() > 0
        assert _real_bits(o) == _real_bits(want)
