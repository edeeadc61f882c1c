"""Every kernel of the training QP (pbd_kernels_qp.hip) on the built inputs of tests/qp_hard_cases.py, byte for byte against the
numpy yardstick QPRef: k_qp_slots and k_qp_write<float / double> on entries of 1 to nearly V values, duplicate offsets, rounding
edges and calls with invalid and foreign headers; k_qp_pass on every outcome of a step (QPRef's `detail`, floors asserted from
the reference that runs beside the device), after every pass; k_qp_lincomb / k_qp_norm on an all-zero dual, ties in a and blocks
that few entries carry; k_qp_score after opt; k_qp_gather on prunes that move nothing, 256 and 257 entries.  No tolerance
anywhere.  tests/test_qp_hard_cpu.py shows on the CPU that a changed rule of the step changes these bytes."""
from collections import Counter

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector
from partsbaseddetector_amd import qp as Q

import qp_hard_cases as H
from test_gpu_qp import same_entries, same_state
from test_qp_hard_cpu import floors_ok

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def handles():
    """one handle per (model, T), made on first use"""
    made = {}

    def get(model, dtype):
        if (model, dtype) not in made:
            made[model, dtype] = detector.Handle(H.MODELS[model](), device=0, real_type=REAL[dtype], max_candidates=1 << 10)
        return made[model, dtype]

    yield get
    for hd in made.values():
        hd.close()


@pytest.fixture(scope="module")
def sets():
    return H.all_sets()


def pair_for(s, hd, capacity=None, **kw):
    """a device QP and a QPRef of set s's configuration"""
    cap = capacity or len(s.hdr) + 8
    cfg = dict(s.cfg)
    cfg.update(kw)
    return Q.QP(hd, cap, **cfg), s.ref(capacity=cap, **kw)


def device_add(q, hd, hdr, vals, rec, label, id_base, count=None, taken=True):
    """headers, values and a payload of `count` records uploaded by the test, into q by pbd_qp_add_device; d_taken"""
    import torch
    m = len(hdr)
    pay = torch.zeros(1 + m * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = m if count is None else count
    pay[1:] = torch.from_numpy(np.ascontiguousarray(rec, np.int32).ravel()).cuda()
    dh = torch.from_numpy(np.ascontiguousarray(hdr, np.int32).ravel()).cuda()
    dv = torch.from_numpy(np.ascontiguousarray(vals, hd.dtype).ravel()).cuda()
    dt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    q.add_device(hd, pay.data_ptr(), m, dh.data_ptr(), dv.data_ptr(), label, id_base, dt.data_ptr() if taken else None)
    return int(dt.item())


def records_for(hd, n, seed=0):
    """n records (only the words an id is made of matter): frames in groups of 1, 3, 4 and 5"""
    ids = H.ids_in_groups(n, 0)
    rec = np.zeros((n, hd.stride), np.int32)
    rec[:, 0] = ids[:, 1]
    rec[:, 2] = ids[:, 2]
    rec[:, 3] = seed
    rec[:, 4] = np.arange(n) % 2
    return rec


# ---- k_qp_write -----------------------------------------------------------------------------------------------------------
# the edge set's halfway and subnormal values are doubles: T = double only
WRITES = [("shapes", np.float32), ("shapes", np.float64), ("dups", np.float32), ("dups", np.float64), ("edges", np.float64)]


@pytest.mark.parametrize("name,dtype", WRITES)
def test_write_host_route(name, dtype, handles, sets):
    s = sets[name]
    hd = handles(s.model, dtype)
    vals = s.values.astype(dtype)
    q, ref = pair_for(s, hd)
    assert q.add(hd, s.hdr, vals, ids=s.ids) == ref.add(s.hdr, vals, s.ids) == len(s.hdr)
    same_entries(q, ref)
    q.close()


@pytest.mark.parametrize("name,dtype", WRITES)
def test_write_device_route(name, dtype, handles, sets):
    s = sets[name]
    hd = handles(s.model, dtype)
    vals = s.values.astype(dtype)
    n = len(s.hdr)
    k = n // 3
    rec = records_for(hd, n, seed=3)
    q, ref = pair_for(s, hd)
    assert device_add(q, hd, s.hdr[:k], vals[:k], rec[:k], 1, 40) == k
    assert device_add(q, hd, s.hdr[k:], vals[k:], rec[k:], -1, 7) == n - k
    ref.add(s.hdr[:k], vals[:k], Q.ids_of_records(rec[:k], 1, 40))
    ref.add(s.hdr[k:], vals[k:], Q.ids_of_records(rec[k:], -1, 7))
    same_entries(q, ref)
    q.close()


@pytest.mark.parametrize("name", ["shapes", "dups"])
def test_write_float_against_double_handles(name, handles, sets):
    """values that float32 holds, through k_qp_write<float> and k_qp_write<double>: the same cache"""
    s = sets[name]
    v32 = s.values.astype(np.float32)
    ref = s.ref()
    ref.add(s.hdr, v32, s.ids)
    got = []
    for dtype in DTYPES:
        hd = handles(s.model, dtype)
        q = Q.QP(hd, len(s.hdr) + 8, **s.cfg)
        assert q.add(hd, s.hdr, v32.astype(dtype), ids=s.ids) == len(s.hdr)
        same_entries(q, ref)
        got.append(q.entries())
        q.close()
    for u, v in zip(*got):
        assert u.tobytes() == v.tobytes()


# ---- k_qp_slots -----------------------------------------------------------------------------------------------------------
def slots_inputs(hd):
    hdr, vals, rec, foreign = H.slots_call(hd.stride)
    vals = vals.astype(hd.dtype)
    lay = Q.Layout(hd.flat)
    valid = np.array([lay.header_ok(h) == 1 for h in hdr])
    assert not valid[list(H.SLOTS_INVALID)].any() and not valid[H.SLOTS_RUN[0]:H.SLOTS_RUN[1]].any()
    assert valid[62] and valid[65] and valid[1025] and valid[H.SLOTS_RUN[1]]
    return hdr, vals, rec, foreign, valid


N0 = 10          # entries the cache holds before the call


def prefilled(hd, s, cap):
    q, ref = Q.QP(hd, cap), Q.QPRef(hd.flat, cap)
    vals = s.values.astype(hd.dtype)
    assert q.add(hd, s.hdr[:N0], vals[:N0], ids=s.ids[:N0]) == ref.add(s.hdr[:N0], vals[:N0], s.ids[:N0]) == N0
    return q, ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_slots_host_route(dtype, handles, sets):
    """the call of 2 100 examples into a cache that holds 10 and fills at example 1032: inside the first wavefront of the second
    round of 1024.  The count taken, the entries and the order of their ids"""
    hd = handles("mixed", dtype)
    hdr, vals, rec, _, valid = slots_inputs(hd)
    cap = N0 + int(valid[:1032].sum())
    assert 1024 < 1032 < 1024 + 64 and valid[1032:].sum() > 0
    q, ref = prefilled(hd, sets["shapes"], cap)
    ids = Q.ids_of_records(rec, -1, 3)
    taken = q.add(hd, hdr, vals, ids=ids)
    assert taken == ref.add(hdr, vals, ids) == cap - N0
    same_entries(q, ref)
    assert np.array_equal(q.entries()[4][N0:], ids[np.nonzero(valid)[0][:taken]])
    q.one(seed=1)
    ref.one(seed=1)
    same_state(q, ref)
    q.close()


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_slots_device_route(dtype, full, handles, sets):
    """the same call on the device, with headers that are not examples of the layout (skipped) and a payload count below the
    capacity (the valid headers past it are ignored).  full: the cache fills at example 1032; otherwise it has room to spare"""
    hd = handles("mixed", dtype)
    hdr, vals, rec, foreign, valid = slots_inputs(hd)
    hdr = hdr.copy()
    lay = Q.Layout(hd.flat)
    for i, h in foreign.items():
        assert valid[i] and lay.header_ok(h) == 0
        hdr[i] = h
        valid[i] = False
    count = H.SLOTS_N - 10
    assert valid[count:].sum() >= 5
    valid[count:] = False
    keep = np.nonzero(valid)[0]
    cap = N0 + (int(valid[:1032].sum()) if full else len(keep) + 5)
    q, ref = prefilled(hd, sets["shapes"], cap)
    ids = Q.ids_of_records(rec, -1, 3)
    want = ref.add(hdr[keep], vals[keep], ids[keep])
    assert want == (cap - N0 if full else len(keep))
    assert device_add(q, hd, hdr, vals, rec, -1, 3, count=count) == want
    assert q.state()["n"] == N0 + want
    same_entries(q, ref)
    assert np.array_equal(q.entries()[4][N0:], ids[keep[:want]])
    q.one(seed=1)
    ref.one(seed=1)
    same_state(q, ref)
    q.close()


# ---- k_qp_pass ------------------------------------------------------------------------------------------------------------
def run_passes(s, hd, count, nfix=0, passes=None, steps=None, **kw):
    """set s on the device and on QPRef side by side: add (the first nfix entries fixed), then the set's passes with the state
    compared after every pass; the reference's details go into count, and (pass, entry, detail) of every step into steps"""
    vals = s.values.astype(hd.dtype)
    q, ref = pair_for(s, hd, **kw)
    if nfix:
        q.add(hd, s.hdr[:nfix], vals[:nfix], ids=s.ids[:nfix])
        ref.add(s.hdr[:nfix], vals[:nfix], s.ids[:nfix])
        q.fix(); ref.fix()
    assert q.add(hd, s.hdr[nfix:], vals[nfix:], ids=s.ids[nfix:]) == ref.add(s.hdr[nfix:], vals[nfix:], s.ids[nfix:])
    same_entries(q, ref)
    for t in range(s.passes if passes is None else passes):
        order = s.order(t, ref.sv)
        S = [i for i in range(ref.n) if ref.sv[i]]
        q.one(order=order)
        ref.one(order=order)
        same_state(q, ref)
        for k, d in zip(order, ref.detail):
            count.update(d)
            if steps is not None:
                steps.append((t, S[int(k)], d))
    return q, ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_pass_on_every_set(dtype, handles, sets):
    count = Counter()
    for name, s in sets.items():
        q, ref = run_passes(s, handles(s.model, dtype), count)
        q.close()
    assert floors_ok(count) == [], dict(count)


@pytest.mark.parametrize("name", ["shapes", "dups"])
def test_pass_with_a_fixed_set(name, handles, sets):
    """the first 12 entries fixed: steps clear the sv of some of them, the end of the pass sets it again (same_state after every
    pass compares sv), so that a cleared fixed entry is stepped again in the next pass"""
    s = sets[name]
    count, steps = Counter(), []
    q, ref = run_passes(s, handles(s.model, np.float64), count, nfix=12, steps=steps)
    assert ref.nfix == 12 and all(ref.sv[:12]) and not all(ref.sv)
    cleared = [(t, i) for t, i, d in steps if i < 12 and "sv_clear" in d]
    assert len(cleared) >= 2, cleared
    assert any((t + 1, i) in {(u, j) for u, j, _ in steps} for t, i in cleared)     # stepped again after the restore
    q.close()


@pytest.mark.parametrize("noneg", ["none", "all"])
def test_pass_noneg_extremes(noneg, handles, sets):
    """no non-negative coordinate, and all L = 9 568 of them (more than the 1 024 lanes of a clamp sweep)"""
    s = sets["shapes_w1"]
    hd = handles(s.model, np.float64)
    L = Q.Layout(hd.flat).L
    nn = np.zeros(0, np.int32) if noneg == "none" else np.arange(L, dtype=np.int32)
    assert L > 1024
    count = Counter()
    q, ref = run_passes(s, hd, count, noneg=nn)
    if noneg == "all":
        assert count["clamp_changed_w_plain"] >= 3 and count["clamp_changed_w_pair"] >= 3 and ref.w.min() == 0.0
    else:
        assert count["clamp_changed_w_plain"] == count["clamp_changed_w_pair"] == 0 and ref.w[ref.lay.noneg].min() < 0
    q.close()


# ---- k_qp_lincomb, k_qp_norm ----------------------------------------------------------------------------------------------
def test_refresh_with_every_dual_zero(handles):
    """b < 0 for every entry (w0 . v > 1): each step finds Ai == 0 and G > 0, so a stays 0: no refresh task at all, w == 0,
    ww == 0, every sv cleared"""
    hd = handles("mixed", np.float64)
    B = H.Blocks(hd.flat)
    ex = [[(B.bias[k], [1.0]), (B.defs[k % len(B.defs)], [-1.0, 1.0, -4.0, 2.0])] for k in range(12)]
    hdr, vals = H.pack(B.lay, ex)
    ids = H.ids_in_groups(12, 4)
    w0 = np.zeros(B.L)
    w0[[b[0] for b in B.bias]] = np.where(np.arange(len(B.bias)) % 2, 2.0, -2.0)      # positives: +v, negatives: -v
    vals[:, 0] = np.where(np.sign(w0[hdr[:, 4]]) == np.sign(ids[:, 0]), 1.0, -1.0)
    q, ref = Q.QP(hd, 16, w0=w0), Q.QPRef(hd.flat, 16, w0=w0)
    assert q.add(hd, hdr, vals, ids=ids) == ref.add(hdr, vals, ids) == 12
    assert all(e.b < 0 for e in ref.e)
    same_entries(q, ref)
    order = np.arange(12, dtype=np.int32)[::-1].copy()
    q.one(order=order)
    ref.one(order=order)
    assert ref.refresh_tasks() == [] and not any(ref.a) and not any(ref.sv) and not ref.w.any() and ref.ww == 0.0
    same_state(q, ref)
    with pytest.raises(detector.PbdError):
        q.one()                                 # no support vector is left
    q.close()


def test_refresh_with_ties_and_rare_blocks(handles, sets):
    """equal duals (the refresh orders them by index) and blocks that only some of the entries with a > 0 carry"""
    count = Counter()
    s = sets["exact"]
    q, ref = run_passes(s, handles(s.model, np.float64), count, passes=1)
    pos = [a for a in ref.a if a > 0]
    assert len(set(pos)) < len(pos) - 2
    q.close()
    s = sets["shapes_w1"]
    q, ref = run_passes(s, handles(s.model, np.float32), count, passes=2)
    pos = [i for i in range(ref.n) if ref.a[i] > 0]
    assert len(set(ref.a[i] for i in pos)) < len(pos)                    # several entries at a == 1
    carriers = Counter(off for i in pos for off, _, _ in ref.e[i].blocks)
    assert 4 * min(carriers.values()) < max(carriers.values())
    f = H.Blocks(handles(s.model, np.float32).flat).filt[1568][0][0]
    assert (f, 1024, 544) in ref.refresh_tasks()
    q.close()


# ---- k_qp_score -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["shapes", "shapes_w1", "one_id"])
def test_scores_and_weights_after_opt(name, dtype, handles, sets):
    s = sets[name]
    hd = handles(s.model, dtype)
    vals = s.values.astype(dtype)
    q, ref = pair_for(s, hd)
    q.add(hd, s.hdr, vals, ids=s.ids)
    ref.add(s.hdr, vals, s.ids)
    st = q.opt(tol=0.01, iter=4, seed=9)
    ref.opt(tol=0.01, iter=4, seed=9)
    assert st["passes"] == ref.passes >= 2 and st["converged"] == ref.converged
    same_state(q, ref)
    got, want = q.scores(), ref.scores()
    assert len(want) == int(np.sum(s.ids[:, 0] > 0)) and got.tobytes() == want.tobytes()
    assert q.weights().tobytes() == ref.weights().tobytes()
    q.close()


# ---- k_qp_gather ----------------------------------------------------------------------------------------------------------
def prune_case(B, moved):
    """one negative whose first step clears its sv (b < 0 under the default w0), then `moved` negatives with one id each that all
    end at a = 1: prune drops entry 0 and moves every other entry down by one"""
    ex = [[(B.defs[0], [-64.0, 0.0, -64.0, 0.0])]]
    for k in range(moved):
        ex.append([(B.bias[1 + k % 9], [1.0])] + ([(B.filt[288][k % 3], 0.01 * H.block_values(B.filt[288][k % 3], k, 1.0))] if k % 50 == 0 else []))
    hdr, vals = H.pack(B.lay, ex)
    ids = np.zeros((len(ex), 5), np.int32)
    ids[:, 0] = -1
    ids[:, 1] = np.arange(len(ex))
    return hdr, vals, ids


@pytest.mark.parametrize("case", ["nothing", "fixed_only", "moves_256", "moves_257"])
def test_prune(case, handles, sets):
    hd = handles("mixed", np.float32)
    B = H.Blocks(hd.flat)
    if case.startswith("moves"):
        moved = int(case.split("_")[1])
        hdr, vals, ids = prune_case(B, moved)
        q, ref = Q.QP(hd, len(hdr), wreg=np.ones(B.L)), Q.QPRef(hd.flat, len(hdr), wreg=np.ones(B.L))
        nfix = 0
    else:
        s = sets["shapes"]
        hdr, vals, ids = s.hdr[:40], s.values[:40], s.ids[:40]
        q, ref = Q.QP(hd, 48), Q.QPRef(hd.flat, 48)
        nfix = 40 if case == "nothing" else 12
    vals = vals.astype(np.float32)
    k = nfix or len(hdr)
    assert q.add(hd, hdr[:k], vals[:k], ids=ids[:k]) == ref.add(hdr[:k], vals[:k], ids[:k]) == k
    if nfix:
        q.fix(); ref.fix()
    if case == "fixed_only":                     # the pass runs before the rest arrives: their a is 0, and every sv is 1
        q.one(seed=5)
        ref.one(seed=5)
    q.add(hd, hdr[k:], vals[k:], ids=ids[k:])
    ref.add(hdr[k:], vals[k:], ids[k:])
    if case != "fixed_only":
        q.one(seed=5)
        ref.one(seed=5)
    same_state(q, ref)
    n0 = ref.n
    before = [e.ids for e in ref.e]
    keep = [i for i in range(n0) if ref.sv[i]] if not all(ref.sv) else [i for i in range(n0) if ref.a[i] > 0 or i < ref.nfix]
    first = next((k for k, i in enumerate(keep) if i != k), len(keep))
    if case == "nothing":
        assert keep == list(range(n0))
    elif case == "fixed_only":
        assert keep == list(range(12)) and n0 == 40
    else:
        assert keep == list(range(1, n0)) and len(keep) - first == moved     # one chunk of 256; 256 + 1
    assert q.prune() == ref.prune() == len(keep)
    assert [e.ids for e in ref.e] == [before[i] for i in keep]
    same_entries(q, ref)
    same_state(q, ref)
    q.one(seed=6)                               # and the compacted cache goes on as the reference's does
    ref.one(seed=6)
    same_state(q, ref)
    q.close()
