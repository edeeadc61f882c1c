"""The training QP's numpy yardstick (partsbaseddetector_amd/qp.py) against things it does not share code with: the literal
sequential-order restatement of the mex pass, weak duality from raw dense examples, and hand-built cases for the paired update,
the non-negativity clamps, lb's monotonicity, prune, the block merge, qp_w and qp_scorepos.  No GPU."""
import numpy as np
import pytest

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd import synth


def random_examples(flat, n, seed, dup=False, dtype=np.float32):
    """n examples of flat's layout (hdr, values in pbd_examples' format): a root bias, some deformation blocks and filter
    blocks; dup: the first filter block repeated (a filter id used twice)"""
    lay = Q.Layout(flat)
    dbase, fbase, L = E.vector_offsets(flat)
    nd = (fbase - dbase) // 4
    hdr = np.zeros((n, lay.in_hw), np.int32)
    vals = np.zeros((n, lay.V), dtype)
    r = synth.randint(seed, 8 * n, 0, 1 << 20, stream=3)
    for i in range(n):
        blocks = [(int(r[8 * i] % dbase), 1)]
        for k in range(2):
            d = int(r[8 * i + 1 + k] % nd)
            if all(b[0] != dbase + 4 * d for b in blocks):
                blocks.append((dbase + 4 * d, 4))
        fs = sorted({int(r[8 * i + 3 + k] % flat.nfilters) for k in range(2)})
        for f in fs:
            blocks.append((fbase + int(flat.filter_offset[f]), int(flat.filter_ksize[f]) ** 2 * flat.flen))
        if dup:
            blocks.append(blocks[-1])
        blocks = blocks[:lay.MB]
        v = []
        for off, ln in blocks:
            if ln == 1:
                v.append(np.ones(1))
            elif ln == 4:
                dx, dy = synth.randint(seed + i, 2, -3, 3, stream=off)
                v.append(np.array([-(dx * dx), -dx, -(dy * dy), -dy], np.float64))
            else:
                v.append(0.25 * synth.normalish(seed * 7919 + i, ln, stream=off))
        v = np.concatenate(v)
        hdr[i, :4] = (i, 0, len(blocks), len(v))
        hdr[i, 4:4 + 2 * len(blocks)] = np.asarray(blocks).ravel()
        vals[i, :len(v)] = v
    return hdr, vals


def ids_for(n, npos, groups=None):
    ids = np.zeros((n, 5), np.int32)
    ids[:, 0] = np.where(np.arange(n) < npos, 1, -1)
    ids[:, 1] = np.arange(n) if groups is None else groups
    return ids


def dense_raw(flat, hdr, vals, ids, C, wpos):
    """raw dense examples, negated for negatives, and each one's C"""
    X = E.densify(hdr, vals, E.vector_offsets(flat)[2])
    lab = ids[:, 0] > 0
    X[~lab] = -X[~lab]
    return X, np.where(lab, C * wpos, C)


MODELS = {"tiny": lambda: M.synthetic_tiny_model(), "face": lambda: M.synthetic_face_model(nparts=8, ncomponents=2)}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_pass_in_header_order_matches_literal_order(name):
    flat = MODELS[name]().flatten()
    hdr, vals = random_examples(flat, 40, 11)
    ids = ids_for(40, 15)    # one id per example: a saturated group's "Ci >= 1" is an exact compare that rounding can flip
    qs = [Q.QPRef(flat, 64, literal=lit) for lit in (False, True)]
    for q in qs:
        assert q.add(hdr, vals, ids) == 40
    rng = np.random.RandomState(3)
    for t in range(4):
        nsv = sum(qs[0].sv)
        order = rng.permutation(nsv)
        for q in qs:
            q.one(order=order)
        assert qs[0].branches == qs[1].branches
        assert qs[0].sv == qs[1].sv
        a0, a1 = np.array(qs[0].a), np.array(qs[1].a)
        assert np.allclose(a0, a1, rtol=1e-9, atol=1e-12)
        scale = np.abs(qs[1].w).max() + 1e-300
        assert np.max(np.abs(qs[0].w - qs[1].w)) <= 1e-9 * scale
        assert abs(qs[0].lb - qs[1].lb) <= 1e-9 * abs(qs[1].lb) + 1e-15
    assert "plain" in qs[0].branches


@pytest.mark.parametrize("name", sorted(MODELS))
def test_opt_weak_duality(name):
    flat = MODELS[name]().flatten()
    hdr, vals = random_examples(flat, 60, 5)
    ids = ids_for(60, 20, groups=np.r_[np.arange(20), 20 + np.arange(40) // 4])
    q = Q.QPRef(flat, 100)
    q.add(hdr, vals, ids)
    q.fix()
    hist = []
    q.opt(tol=0.05, iter=200, seed=1, history=hist)
    assert q.converged and q.lb > 0
    assert 1 - q.lb / q.ub < 0.05
    X, Cs = dense_raw(flat, hdr, vals, ids, 0.002, 2.0)
    p = Q.primal(X, [tuple(r) for r in ids], Cs, q.wreg, q.w0, q.w)
    eps = 1e-5 * abs(p)
    assert q.lb <= p + eps and p <= q.ub + eps, (q.lb, p, q.ub)
    lbs = [h["lb"] for h in hist]
    assert all(b > a - 1e-5 for a, b in zip(lbs, lbs[1:]))
    assert q.lb_dropped == 0


def test_paired_update_through_idI():
    """two negatives with one id whose group saturates: the second step moves dual mass through idI"""
    flat = M.synthetic_tiny_model().flatten()
    hdr, vals = random_examples(flat, 2, 9)
    vals = vals * 0.25      # |x'|^2 small against b: the first step saturates the group (a = 1)
    ids = np.array([[-1, 7, 0, 0, 0]] * 2, np.int32)
    ones = np.ones(E.vector_offsets(flat)[2])   # no root-bias weighting: d stays small
    q = Q.QPRef(flat, 4, wreg=ones)
    q.add(hdr, vals, ids)
    q.one(order=[0, 1])
    assert q.branches[0] == "plain"       # a0 = 1: the group saturates
    assert q.branches[1] == "pair"
    assert 0 < q.a[1] <= 1 and abs(q.a[0] + q.a[1] - 1.0) < 1e-12
    lit = Q.QPRef(flat, 4, wreg=ones, literal=True)
    lit.add(hdr, vals, ids)
    lit.one(order=[0, 1])
    assert lit.branches == q.branches
    assert np.allclose(lit.a, q.a, rtol=1e-9)


def test_nonnegativity_clamps_fire():
    flat = M.synthetic_tiny_model().flatten()
    dbase, fbase, L = E.vector_offsets(flat)
    lay = Q.Layout(flat)
    hdr = np.zeros((1, lay.in_hw), np.int32)
    vals = np.zeros((1, lay.V), np.float32)
    hdr[0, :6] = (0, 0, 1, 4, dbase, 4)
    vals[0, :4] = (-4, -2, -9, -3)      # -dx^2, -dx, -dy^2, -dy of a positive: w . x grows as w[0], w[2] fall
    q = Q.QPRef(flat, 2)
    q.add(hdr, vals, [[1, 0, 0, 0, 0]])
    q.one(order=[0])
    assert q.branches == ["plain"] and q.a[0] > 0
    unclamped = q.a[0] * q.e[0].x.astype(np.float64)
    assert unclamped[0] < 0 and unclamped[2] < 0
    assert q.w[dbase] == 0.0 and q.w[dbase + 2] == 0.0
    assert q.w[dbase + 1] == unclamped[1] and q.w[dbase + 3] == unclamped[3]


def test_prune_keeps_fixed_and_order():
    flat = M.synthetic_tiny_model().flatten()
    hdr, vals = random_examples(flat, 30, 21)
    q = Q.QPRef(flat, 40)
    q.add(hdr[:8], vals[:8], ids_for(8, 8))
    q.fix()
    ids = ids_for(22, 0)
    ids[:, 1] += 100
    q.add(hdr[8:], vals[8:], ids)
    q.one(seed=4)
    before = [e.ids for e in q.e]
    keep = [i for i in range(q.n) if q.sv[i]] if not all(q.sv) else \
        [i for i in range(q.n) if q.a[i] > 0 or i < q.nfix]
    n = q.prune()
    assert n == len(keep) and [e.ids for e in q.e] == [before[i] for i in keep]
    assert q.nfix == 8 and [e.ids for e in q.e[:8]] == before[:8]
    assert all(q.sv)


def test_merge_of_duplicate_blocks_keeps_wx():
    flat = M.synthetic_tiny_model().flatten()
    hdr, vals = random_examples(flat, 5, 13, dup=True)
    w = E.model_vector(flat, np.float64)
    q = Q.QPRef(flat, 8, wreg=np.ones(len(w)))
    q.add(hdr, vals, ids_for(5, 5))
    for i, e in enumerate(q.e):
        offs = [b[0] for b in e.blocks]
        assert len(offs) == len(set(offs)) == hdr[i, 2] - 1
        merged = float(np.dot(w[e.idx], e.x.astype(np.float64))) / q.Cpos
        raw = float(E.dot(hdr[i], vals[i], w)[0])
        assert abs(merged - raw) <= 1e-6 * (E.abs_dot(hdr[i], vals[i], w)[0] + 1e-30)


def test_qp_w_and_scorepos():
    flat = M.synthetic_tiny_model().flatten()
    hdr, vals = random_examples(flat, 12, 17)
    ids = ids_for(12, 7)
    q = Q.QPRef(flat, 16)
    q.add(hdr, vals, ids)
    wm = E.model_vector(flat, np.float64)
    q.w = (wm - q.w0) * q.wreg          # model2vec's scaling (train.m: qp.w = (w - w0) .* wreg)
    assert np.allclose(q.weights(), wm, rtol=1e-15, atol=1e-15)
    s = q.scores()
    want = E.dot(hdr[:7], vals[:7], wm)
    bound = 1e-6 * E.abs_dot(hdr[:7], vals[:7], wm) + 1e-12
    assert len(s) == 7 and np.all(np.abs(s - want) <= bound)


def test_reduction_order_is_pinned():
    """R is the lane-strided sum then the two halving trees, not a plain sum (a case where they differ)"""
    p = np.zeros(2048)
    p[0], p[1024], p[1] = 1.0, 1e-16, -1.0
    assert Q.reduce_r(p) == 0.0          # lane 0: 1 + 1e-16 = 1; the tree then cancels lane 1
    assert Q.reduce_seq(p) == 1e-16
    assert Q.reduce_r(np.zeros(0)) == 0.0


def test_seeded_order_is_stable_argsort_of_splitmix():
    o = Q.seeded_order(5, 100)
    assert sorted(o.tolist()) == list(range(100))
    z = synth.splitmix64(5, 100)
    assert np.all(np.diff(z[o].astype(np.float64)) >= 0)
