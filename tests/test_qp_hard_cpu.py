"""What the built QP inputs of tests/qp_hard_cases.py reach, on the numpy yardstick alone (no GPU): every outcome of a step of
qp_one_sparse that QPRef's `detail` names has its floor, the entries have the sizes the kernels' edges need, the exact cases are
the cases they are built to be, and a QPRef with any single rule of the step changed ends in another state on some set -- the
evidence that a kernel carrying that change would fail the byte comparisons of tests/test_gpu_qp_hard.py.  The counts measured
when the sets were built are in DESIGN.md section 6i; the tests assert floors."""
from collections import Counter

import numpy as np
import pytest

from partsbaseddetector_amd import qp as Q

import qp_hard_cases as H

# labels the sets are built to reach (floor 3) and labels that need an exact tie or an exact zero (floor 1)
FLOOR3 = ["plain_free", "plain_floor0", "plain_cap_maxA", "pair_up_free", "pair_up_bound_A2", "pair_down_free", "pair_down_bound_-Ai",
          "pair_G_zeroed", "pair_small_G", "none_lower", "none_upper", "i2_is_i", "sv_clear", "err_raised", "clamp_changed_w_plain",
          "clamp_changed_w_pair", "pair_blocks_i2_lacks", "pair_blocks_i2_extra", "pair_blocks_shifted"]
FLOOR1 = ["pair_up_bound_1-Ai", "pair_down_bound_A2-1", "G_is_0"]


def floors_ok(count):
    return [l for l in FLOOR3 if count[l] < 3] + [l for l in FLOOR1 if count[l] < 1]


@pytest.fixture(scope="module")
def runs():
    """every set run once on QPRef: name -> (set, final QPRef, details of every step, snapshots after every pass)"""
    out = {}
    for name, s in H.all_sets().items():
        snaps = []
        q, det = H.run_ref(s, each=lambda t, q: snaps.append(q.snapshot()))
        out[name] = (s, q, det, snaps)
    return out


def test_every_outcome_is_reached(runs):
    count = Counter()
    for s, q, det, _ in runs.values():
        for d in det:
            count.update(d)
    assert floors_ok(count) == [], dict(count)
    known = set(FLOOR3) | set(FLOOR1)
    assert set(count) <= known, set(count) - known
    # the sets that the GPU pass test runs on their own
    for name in ("shapes_w1", "dups"):
        c = Counter(l for d in runs[name][2] for l in d)
        assert c["pair_up_free"] >= 3 and c["pair_down_free"] >= 3 and c["pair_G_zeroed"] >= 3, (name, dict(c))


def test_branches_agree_with_detail(runs):
    """`branches` is what it was: a step is "plain" or "pair" exactly when detail names a plain or a paired outcome"""
    for name, (s, q, _, _) in runs.items():
        assert len(q.branches) == len(q.detail) > 0
        for b, d in zip(q.branches, q.detail):             # the last pass
            kind = {l.split("_")[0] for l in d if l.split("_")[0] in ("plain", "pair") and not l.startswith("pair_blocks")
                    and l not in ("pair_small_G", "pair_G_zeroed")}
            assert kind == ({b} if b != "none" else set()), (name, b, d)


def test_entry_sizes_and_layout_edges(runs):
    s, q, _, _ = runs["shapes"]
    lay = q.lay
    assert (lay.V, lay.MB, lay.L) == (5520, 11, 9568)
    assert sorted({ln for _, ln in lay.blocks}) == [1, 4, 288, 512, 800, 1568]
    nv = {len(e.x) for e in q.e}
    assert {1, 4, 5, 16, 288, 1024, 1025, 1573, 2080, 5519} <= nv
    B = H.Blocks(H.mixed_model().flatten())
    assert H.nearest_nv(B, 2048) == 2080 and H.nearest_nv(B, lay.V) == lay.V    # 2048 itself is not an entry size of this layout
    by_nv = {len(e.x): e for e in q.e}
    assert all(ln != 1 for _, ln, _ in by_nv[288].blocks + by_nv[1024].blocks)          # no bias block
    assert len(by_nv[5519].blocks) == lay.MB
    assert any(st > 1024 and st % 1024 for e in q.e for _, _, st in e.blocks)           # k_qp_write's lane rotation
    assert by_nv[2080].blocks[1][2] == 1568
    # groups of 1, 3, 4 and 5 negatives; positives one id each
    sizes = Counter(Counter(e.ids for e in q.e if e.ids[0] < 0).values())
    assert {1, 3, 4, 5} <= set(sizes)
    assert set(Counter(e.ids for e in q.e if e.ids[0] > 0).values()) == {1}
    # entries with a > 0 carry a 1568-value block, which the refresh splits as 1024 + 544: a property of the inputs (refresh_tasks
    # restates the host's split; on the device the bytes of w guard it)
    f = B.filt[1568][0][0]
    tasks = q.refresh_tasks()
    assert (f, 0, 1024) in tasks and (f, 1024, 544) in tasks
    assert all(0 < n <= 1024 for _, _, n in tasks)


def test_duplicate_offsets_merge():
    s = H.dup_set()
    q = s.ref()
    q.add(s.hdr, s.values, s.ids)
    B = H.Blocks(H.mixed_model().flatten())
    A = B.filt[288][0]
    times = [[int(h[4 + 2 * b]) for b in range(h[2])] for h in s.hdr]
    assert any(t.count(A[0]) == 3 and t[0] == A[0] for t in times)                     # three times, and as the first block
    assert any(t[1:4] == [A[0], B.filt[512][0][0], A[0]] for t in times)              # A B A
    assert any(t.count(B.defs[0][0]) >= 2 for t in times)                              # a duplicated deformation block
    for e, t in zip(q.e, times):
        offs = [b[0] for b in e.blocks]
        assert offs == list(dict.fromkeys(t))                                          # one block per offset, first-use order
        assert len(e.x) == sum(b[1] for b in e.blocks) == sum(q.lay.slot_len[o] for o in dict.fromkeys(t))


def test_exact_cases(runs):
    """the power-of-two set steps exactly as its docstring says, in detail's words"""
    s = H.exact_set()
    at = {n: k for k, n in enumerate(s.names)}
    q = s.ref()
    q.add(s.hdr, s.values, s.ids)
    q.one(order=s.order(0, q.sv))
    d1 = {s.names[k]: d for k, d in zip(s.orders[0], q.detail)}
    assert "plain_free" in d1["E"] and q.a[at["E"]] == 0.5
    assert {"G_is_0", "none_lower"} <= d1["E2"] and "sv_clear" not in d1["E2"] and q.sv[at["E2"]] == 1
    assert "plain_cap_maxA" in d1["S"]                                                  # Ci == 1 by one saturating step ...
    assert {"pair_up_bound_1-Ai", "pair_up_bound_A2"} <= d1["T"]                      # ... and dA == 1 == both bounds
    assert (q.a[at["S"]], q.a[at["T"]]) == (0.0, 1.0)
    assert "plain_free" in d1["H1"] and "plain_cap_maxA" in d1["H2"]                  # 1/2 + 1/2
    assert "pair_up_free" in d1["H3"] and q.a[at["H1"]] + q.a[at["H2"]] + q.a[at["H3"]] == 1.0
    assert "pair_up_free" in d1["Q"] and (q.a[at["P"]], q.a[at["Q"]], q.a[at["Z"]]) == (0.5, 0.5, 1.0)
    assert q.sv == [1] * len(s.names)
    q.one(order=s.order(1, q.sv))
    d2 = {s.names[k]: d for k, d in zip(s.orders[1], q.detail)}
    assert "G_is_0" in d2["E"] and not any(l.startswith(("plain", "pair")) for l in d2["E"])
    assert {"pair_down_bound_-Ai", "pair_down_bound_A2-1"} <= d2["Q"]
    assert (q.a[at["P"]], q.a[at["Q"]]) == (1.0, 0.0)
    # every value of the set's state sits on the grid: the literal summation order gives the same bytes
    lit, _ = H.run_ref(s, q=s.ref(literal=True))
    ref = runs["exact"][1]
    assert np.array(lit.a).tobytes() == np.array(ref.a).tobytes() and lit.w.tobytes() == ref.w.tobytes()


def test_write_edges_are_halfway_cases():
    """the edge set's x' of its halfway values: the unrounded quotient lies exactly between two floats, the kept bit takes both
    parities, and subnormal results occur"""
    s = H.edge_set()
    q = s.ref()
    q.add(s.hdr, s.values, s.ids)
    e = q.e[3]                                   # a negative: x' = (C * -v) / wreg
    k0 = [st for off, ln, st in e.blocks if ln == 288][0]
    exact = (q.Cneg * -np.asarray(s.values[3, 5:5 + 288], np.float64)) / q.wreg[e.idx[k0:k0 + 288]]
    x = e.x[k0:k0 + 288].astype(np.float64)
    lo, hi = np.nextafter(e.x[k0:k0 + 288], np.float32(-np.inf)).astype(np.float64), np.nextafter(e.x[k0:k0 + 288], np.float32(np.inf)).astype(np.float64)
    half = (exact != x) & ((exact - lo == x - exact) | (hi - exact == exact - x))
    assert half.sum() >= 16
    bits = e.x[k0:k0 + 288].view(np.uint32)
    assert np.all(bits[half] % 2 == 0)                                                  # ties went to even ...
    up, down = half & (np.abs(x) > np.abs(exact)), half & (np.abs(x) < np.abs(exact))   # ... by rounding up and by rounding down
    assert up.sum() >= 3 and down.sum() >= 3
    tiny = np.float64(np.finfo(np.float32).tiny)
    assert np.sum((x != 0) & (np.abs(x) < tiny)) >= 4                                   # subnormal x'
    assert np.any(q.wreg < 0) and np.any((q.wreg != 1) & (q.wreg > 0)) and np.any(q.w0[e.idx[k0:k0 + 288]] != 0)


# ---- sensitivity: one rule changed at a time ----------------------------------------------------------------------------------
def variant(**methods):
    return type("Changed", (Q.QPRef,), methods)


def _err_late(self, err, j, G, det):
    if -G > err[j]:
        err[j] = -G


def _pair_no_clamp(self, dA, i, i2):
    self._axpy(dA, i)
    self._axpy(-dA, i2)
    return False


def _pair_clamp_early(self, dA, i, i2):
    self._axpy(dA, i)
    c = self._clamp()
    self._axpy(-dA, i2)
    return c


def _idI_always(self, idI, j, i):
    idI[j] = i


CHANGED = {
    "sv clear with >=": variant(_clears_sv=lambda self, Ai, G: Ai == 0 and G >= 0),
    "Ci > 1 for Ci >= 1": variant(_saturated=lambda self, Ci: Ci > 1),
    "Ci > 1 for Ci >= 1 in none_upper alone": variant(_is_upper=lambda self, Ci, G: Ci > 1 and G <= 0),
    "Ci > 1 for Ci >= 1 in the paired path's condition alone": variant(_pair_saturated=lambda self, Ci: Ci > 1),
    "paired path zeroes G with >=": variant(_pair_zeroes_G=lambda self, Ai, G: Ai == 0 and G >= 0),
    "no floor at 0 (plain)": variant(_plain_floor=lambda self, x: x),
    "no cap at maxA (plain)": variant(_plain_cap=lambda self, x, maxA: x),
    "no bound A2 (pair, dA > 0)": variant(_pair_up_other=lambda self, dA, A2: dA),
    "no bound -Ai (pair, dA <= 0)": variant(_pair_down_own=lambda self, dA, Ai: dA),
    "no bound A2 - 1 (pair, dA <= 0)": variant(_pair_down_other=lambda self, dA, A2: dA),
    "1e-12 -> 0": variant(EPS=0.0),
    "1e-12 -> 1e-9": variant(EPS=1e-9),
    "no clamp after a paired update": variant(_pair_update=_pair_no_clamp),
    "clamp before the second axpy": variant(_pair_update=_pair_clamp_early),
    "idI = i also when a[i] == 0": variant(_note_idI=_idI_always),
    "err after the step": variant(_note_err=lambda self, err, j, G, det: None, _note_err_late=_err_late),
    "refresh in index order": variant(_refresh_order=lambda self: [i for i in range(self.n) if self.a[i] > 0]),
}

# Rules that cannot change the state (DESIGN.md section 6i gives each argument):
#  none_lower with >, none_upper with <: they differ from >= and <= only at G == 0, where PG = G = 0 either way: no step.
#  no i2 != i: the paired path with i2 == i forms G - G = 0: no step; the plain path is closed too, since Ci >= 1 and G < 0 make
#      PG = 0.  Neither clears sv (G < 0).
#  no bound 1 - Ai: a group's duals sum to at most 1, so A2 <= 1 - Ai: the bound A2 is at least as tight.  Rounding can push
#      a group's sum an ulp past 1 (that is how "no bound A2 - 1" changes the state of shapes_w1: Ai = 2^-55 beside A2 = 1), but then
#      1 - Ai still rounds to 1 >= A2; no set has both duals inside (0, 1) with a sum past 1.
#  paired path keeps G > 0: it is taken with Ai == 0, so a G > 0 left in place gives dA < 0, which the bound -Ai = -0 holds at
#      -0: a[i], a[i2] and w (never -0 itself) come out as they were, and sv is cleared in either case.
NO_EFFECT = {
    "none_lower with >": variant(_is_lower=lambda self, Ai, G: Ai == 0 and G > 0),
    "none_upper with <": variant(_is_upper=lambda self, Ci, G: self._saturated(Ci) and G < 0),
    "no i2 != i": variant(_other=lambda self, i2, i: True),
    "no bound 1 - Ai (pair, dA > 0)": variant(_pair_up_own=lambda self, dA, Ai: dA),
    "paired path keeps G > 0": variant(_pair_zeroed_G=lambda self, G: G),
}


def state_bytes(q):
    return (np.array(q.a).tobytes(), bytes(q.sv), q.w.tobytes(), np.float64([q.lb, q.ub, q.loss]).tobytes())


def differs_on(cls, runs, **kw):
    """the sets on which cls ends in a state other than QPRef's (a, sv, w, lb, ub or loss)"""
    out = []
    for name, (s, q, _, _) in runs.items():
        with np.errstate(all="ignore"):
            c, _ = H.run_ref(s, q=s.ref(cls, **kw))
        if state_bytes(c) != state_bytes(q):
            out.append(name)
    return out


@pytest.mark.parametrize("rule", sorted(CHANGED))
def test_a_changed_rule_changes_the_state(rule, runs):
    assert differs_on(CHANGED[rule], runs) != [], rule


def test_sequential_sums_change_the_state(runs):
    """R replaced by the sequential sum (QPRef(literal=True)): other bytes on the sets with long entries"""
    assert "shapes" in differs_on(Q.QPRef, runs, literal=True)


@pytest.mark.parametrize("rule", sorted(NO_EFFECT))
def test_rules_without_effect(rule, runs):
    assert differs_on(NO_EFFECT[rule], runs) == [], rule


# ---- the literal restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_id", "exact", "edges"])
def test_literal_order_gives_the_same_steps(name, runs):
    """on the sets without a saturated group of several entries whose exact compare rounding could flip (and on the exact grid),
    sequential sums take the same steps: equal detail, a and w within 1e-9"""
    s = H.all_sets()[name]
    assert not s.tie_sensitive
    if name == "edges":     # its group of three never fills: no step meets Ci >= 1
        assert not any(l == "none_upper" or l.startswith("pair") for d in runs[name][2] for l in d)
    qs = [s.ref(), s.ref(literal=True)]
    for q in qs:
        q.add(s.hdr, s.values, s.ids)
    for t in range(s.passes):
        order = s.order(t, qs[0].sv)
        for q in qs:
            q.one(order=order)
        assert qs[0].detail == qs[1].detail and qs[0].branches == qs[1].branches
        assert qs[0].sv == qs[1].sv
        assert np.allclose(qs[0].a, qs[1].a, rtol=1e-9, atol=1e-12)
        scale = np.abs(qs[1].w).max() + 1e-300
        assert np.max(np.abs(qs[0].w - qs[1].w)) <= 1e-9 * scale
        assert abs(qs[0].lb - qs[1].lb) <= 1e-9 * abs(qs[1].lb) + 1e-15
