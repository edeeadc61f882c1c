"""CPU tests of training's yardsticks: QPRef.clear / QPRef.add_loss (partsbaseddetector_amd/qp.py) and train_ref
(partsbaseddetector_amd/train.py) on the two cases of tests/train_cases.py -- the branches each run must reach, the final bounds
and the threshold's order statistic."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import train as T
from partsbaseddetector_amd.qp import QPRef, reduce_r

import train_cases as TC


def _examples(flat, n, seed):
    """n random placements' examples of the tiny model on a random feature map"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((8, 10 * 32)).astype(np.float32)
    H, V, ids = [], [], []
    for i in range(n):
        pl = [(int(rng.integers(10)), int(rng.integers(8)), int(rng.integers(2))) for _ in range(3)]
        h, v = E.example(flat, feat, 0, pl, i)
        H.append(h)
        V.append(v)
        ids.append((1 if i < 3 else -1, i // 2, 0, i, 0))
    return np.array(H), np.array(V), np.array(ids, np.int32)


def test_clear_then_the_same_adds_equals_a_fresh_qp():
    flat = M.synthetic_tiny_model().flatten()
    H, V, ids = _examples(flat, 9, 1)
    q = QPRef(flat, 16)
    q.add(H[::-1], V[::-1], ids[::-1])
    q.fix()
    q.opt(0.05, 5, 3)
    assert q.n == 9 and q.nfix == 9 and q.lb == q.lb
    q.clear()
    assert (q.n, q.nfix, q.l, q.loss) == (0, 0, 0.0, 0.0) and q.lb != q.lb and q.ub != q.ub
    q.add(H, V, ids)
    fresh = QPRef(flat, 16)
    fresh.add(H, V, ids)
    for a, b in zip(q.entries(), fresh.entries()):
        assert a.tobytes() == b.tobytes()
    assert q.a == fresh.a and q.sv == fresh.sv
    q.fix(); fresh.fix()
    q.opt(0.05, 5, 3); fresh.opt(0.05, 5, 3)
    assert (q.lb, q.ub) == (fresh.lb, fresh.ub) and q.w.tobytes() == fresh.w.tobytes()


def _records(scores):
    rec = np.zeros((len(scores), 20), np.int32)
    rec[:, 5] = np.asarray(scores, np.float32).view(np.int32)
    return rec


def _ready(flat):
    H, V, ids = _examples(flat, 6, 2)
    q = QPRef(flat, 16)
    q.add(H, V, ids)
    q.fix()
    q.one(seed=1)
    return q


@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 5000])
def test_add_loss_is_the_hinge_sum(n):
    flat = M.synthetic_tiny_model().flatten()
    q = _ready(flat)
    rng = np.random.default_rng(n)
    s = (rng.standard_normal(n) * 1.5 - 1.0).astype(np.float32)
    if n > 2:
        s[1], s[2] = -1.0, np.nextafter(np.float32(-1), np.float32(0))
    ub0 = q.ub
    added = q.add_loss(_records(s), -1)
    seq = 0.0
    for v in s:
        seq += max(0.0, 1.0 + float(v))
    assert abs(added - q.Cneg * seq) <= 1e-12 * max(abs(q.Cneg * seq), 1e-300)
    assert q.ub == ub0 + added
    pos = q.add_loss(_records(s), 1)
    seq = 0.0
    for v in s:
        seq += max(0.0, 1.0 - float(v))
    assert abs(pos - q.Cpos * seq) <= 1e-12 * max(abs(q.Cpos * seq), 1e-300)


def test_add_loss_changes_when_a_rule_is_altered():
    flat = M.synthetic_tiny_model().flatten()
    s = np.array([-3.0, -1.0, -0.5, 0.25, 2.0, -1.5], np.float32)
    base = _ready(flat).add_loss(_records(s), -1)

    class NoFloor(QPRef):
        def _hinge(self, y, score):
            return 1.0 - y * score

    class WrittenOnly(QPRef):
        def _loss_records(self, records):
            return records[:max(self.cap - self.n, 0)]

    for cls in (NoFloor, WrittenOnly):
        H, V, ids = _examples(flat, 6, 2)
        q = cls(flat, 8)
        q.add(H, V, ids)
        q.fix()
        q.one(seed=1)
        assert q.add_loss(_records(s), -1) != base, cls.__name__
    with pytest.raises(ValueError):
        QPRef(flat, 8).add_loss(_records(s), -1)


@pytest.fixture(scope="module")
def latent_run(oracle):
    model, pos, neg, kw = TC.latent_case()
    return T.train_ref(model, pos, neg, 0, **kw)


def test_train_ref_latent_case_reaches_every_branch(latent_run):
    model, info = latent_run
    _, pos, neg, kw = TC.latent_case()
    assert info["numpositives"] == [len(pos)] and not info["skipped"] and not info["notfound"]
    branches = [b["branch"] for b in info["batches"]]
    assert any(b["branch"] == "opt+prune" and b["taken"] + b0 == kw["capacity"]
               for b, b0 in zip(info["batches"], [info["numpositives"][0]] + [b["n"] for b in info["batches"]]))
    assert "one" in branches
    assert any(b["dropped"] > 0 for b in info["batches"])
    assert info["lb"] > 0 and info["ub"] >= info["lb"]
    assert model.thresh == info["thresh"]


def test_train_ref_threshold_is_the_order_statistic(oracle):
    """the threshold is r[ceil(0.05 n) - 1] of the sorted positive scores of the final QP, as float"""
    assert T.threshold_of([3.0, 1.0, 2.0]) == 1.0
    r = np.arange(100, 0, -1.0)
    assert T.threshold_of(r) == 5.0 and T.threshold_of(r[:41]) == float(np.sort(r[:41])[math.ceil(0.05 * 41) - 1])
    model, pos, neg, kw = TC.warp_case()
    out, info = T.train_ref(model, pos, neg, 1, **kw)
    assert info["skipped"] == [3] and info["numpositives"] == [len(pos) - 1] and not info["notfound"]
    assert any(b["branch"] == "opt+prune" for b in info["batches"]) and any(b["dropped"] > 0 for b in info["batches"])
    assert info["lb"] > 0 and out.thresh == info["thresh"]
    # the trained model scores its own positives: the threshold is the lowest of the 5 scores, from the model's own vector
    from partsbaseddetector_amd import warp as W
    flat = out.flatten()
    boxes = np.array([[i, *p["boxes"][0]] for i, p in enumerate(pos)], np.int32)
    H, V, kept = W.warp_examples(flat, [p["im"] for p in pos], boxes, 0, 0, True)
    s = E.dot(H[kept == 1], V[kept == 1], out.to_vector(np.float64))
    assert abs(float(np.sort(s)[0]) - info["thresh"]) <= 1e-5


def test_train_ref_second_iteration_and_double(oracle):
    model, pos, neg, kw = TC.latent_case()
    out, info = T.train_ref(model, pos, neg, 0, iters=2, **kw)
    assert len(info["iterations"]) == 2 and info["iterations"][1]["numpositives"] == [len(pos)]
    assert info["lb"] > 0
    out64, info64 = T.train_ref(model, pos, neg, 0, dtype=np.float64, **kw)
    assert info64["lb"] > 0 and [b["branch"] for b in info64["batches"]]


def test_croppos_and_batches():
    im = np.zeros((72, 96, 3), np.uint8)
    boxes = np.array([[40, 30, 49, 41], [44, 36, 55, 45]], np.int64)
    crop, bx = T.croppos(im, boxes)
    # union 40..55 x 30..45: pad = 0.5 * (16 + 16) = 16 -> columns 24..71, rows 14..61
    assert crop.shape[:2] == (48, 48) and np.shares_memory(crop, im)
    assert np.array_equal(bx, boxes - [24, 14, 24, 14])
    crop, bx = T.croppos(im, np.array([[2, 3, 90, 60]], np.int64))
    assert crop.shape[:2] == (72, 96) and np.array_equal(bx, [[2, 3, 90, 60]])
    pos = [{"boxes": [[0, 0, 19, 19]]}, {"boxes": [[0, 0, 19, 19]]}, {"boxes": [[0, 0, 18, 19]]}, {"boxes": [[0, 0, 30, 30]]}]
    assert T.positive_batches(pos, 5, 4, 8) == ([2], [[0, 1], [3]])
    assert T.positive_batches(pos[:2] + pos[3:], 5, 4, 2) == ([], [[0, 1], [2]])
