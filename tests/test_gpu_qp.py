"""The training QP on the device (pbd_qp_*), bit for bit against the numpy yardstick QPRef (partsbaseddetector_amd/qp.py): cache
writes from host and device examples of float and double handles (person, shared-filter and 3-component models), a full cache,
passes with explicit orders, seeded opt, prune, scores and weights; the QP outliving its handle; refusals; and an end-to-end
round (latent positives + hard negatives -> opt -> a new model vector that loads into a new handle)."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def shared_model():
    m = M.synthetic_tiny_model(thresh=-1.0)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def records(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], _lib.DEPTH_CODE[fr[0].dtype], buf.ctypes.data,
                                      hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


MODELS = {"person": lambda: M.synthetic_person_model(thresh=-100.0), "shared": shared_model,
          "face3": lambda: M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0)}
SIZES = {"person": (120, 160), "shared": (72, 96), "face3": (64, 80)}


def mined(name, dtype, n=48, seed=2):
    """(model, handle, records, hdr, values) of n records of one synthetic frame"""
    model = MODELS[name]()
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 18)
    im = synth.synthetic_frame(seed, *SIZES[name])
    rec = records(hd, [im])
    rec = rec[np.random.default_rng(seed).permutation(len(rec))[:n]]
    hdr, vals = hd.examples(rec)
    return model, hd, rec, hdr, vals


def same_entries(q, ref):
    H, X, b, d, ids = q.entries()
    rH, rX, rb, rd, rids = ref.entries()
    assert np.array_equal(H, rH)
    assert np.array_equal(ids, rids)
    assert b.tobytes() == rb.tobytes() and d.tobytes() == rd.tobytes()
    assert X.tobytes() == rX.tobytes()


def same_state(q, ref):
    s = q.state(arrays=True)
    assert s["n"] == ref.n
    assert s["a"].tobytes() == np.array(ref.a).tobytes()
    assert np.array_equal(s["sv"], np.array(ref.sv, np.uint8))
    assert s["w"].tobytes() == ref.w.tobytes()
    for k in ("lb", "ub", "loss", "l"):
        assert np.float64(s[k]).tobytes() == np.float64(getattr(ref, k)).tobytes(), (k, s[k], getattr(ref, k))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_add_bit_for_bit(name, dtype):
    model, hd, rec, hdr, vals = mined(name, dtype)
    flat = model.flatten()
    npos = len(rec) // 3
    q = Q.QP(hd, 64)
    ref = Q.QPRef(flat, 64)
    assert q.add(hd, hdr[:npos], vals[:npos], rec[:npos], label=1, id_base=10) == npos
    assert q.add(hd, hdr[npos:], vals[npos:], rec[npos:], label=-1, id_base=10) == len(rec) - npos
    ref.add(hdr[:npos], vals[:npos], Q.ids_of_records(rec[:npos], 1, 10))
    ref.add(hdr[npos:], vals[npos:], Q.ids_of_records(rec[npos:], -1, 10))
    same_entries(q, ref)
    hd.close()


def device_add(q, hd, rec, hdr_words, vw, dtype, label, id_base=0):
    """examples of rec on the device (pbd_examples_device) into q (pbd_qp_add_device); the count the call reports"""
    import torch
    st = hd.stride
    pay = torch.zeros(1 + len(rec) * st, dtype=torch.int32, device="cuda")
    pay[0] = len(rec)
    pay[1:] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
    dh = torch.zeros(len(rec) * hdr_words, dtype=torch.int32, device="cuda")
    dv = torch.zeros(len(rec) * vw, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    dt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    hd.examples_device(pay.data_ptr(), len(rec), 0, dh.data_ptr(), dv.data_ptr())
    q.add_device(hd, pay.data_ptr(), len(rec), dh.data_ptr(), dv.data_ptr(), label, id_base, dt.data_ptr())
    return int(dt.item())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_full_cache_and_device_path_equals_host_path(name, dtype):
    model, hd, rec, hdr, vals = mined(name, dtype, n=40)
    flat = model.flatten()
    hw, vw = hd.example_stride()
    cap = 32
    qh, qd = Q.QP(hd, cap), Q.QP(hd, cap)
    ref = Q.QPRef(flat, cap)
    assert qh.add(hd, hdr[:20], vals[:20], rec[:20], label=1, id_base=5) == 20
    assert qh.add(hd, hdr[20:], vals[20:], rec[20:], label=-1, id_base=5) == 12       # only what fits
    assert device_add(qd, hd, rec[:20], hw, vw, dtype, 1, 5) == 20
    assert device_add(qd, hd, rec[20:], hw, vw, dtype, -1, 5) == 12
    ref.add(hdr[:20], vals[:20], Q.ids_of_records(rec[:20], 1, 5))
    ref.add(hdr[20:], vals[20:], Q.ids_of_records(rec[20:], -1, 5))
    same_entries(qd, ref)
    a, b = qh.entries(), qd.entries()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    # a full cache takes nothing more and its entries stay as they were
    assert device_add(qd, hd, rec[:8], hw, vw, dtype, 1, 99) == 0
    assert qh.add(hd, hdr[:8], vals[:8], rec[:8], label=1, id_base=99) == 0
    for q in (qh, qd):
        assert q.state()["n"] == cap
        for u, v in zip(q.entries(), b):
            assert u.tobytes() == v.tobytes()
        with pytest.raises(PbdError):
            q.entries(cap, 1)
    qh.fix(); qd.fix()
    for q in (qh, qd):
        q.one(order=np.arange(cap)[::-1].copy())
    assert qh.state(arrays=True)["w"].tobytes() == qd.state(arrays=True)["w"].tobytes()
    hd.close()


def test_prune_in_several_chunks():
    """a cache of 3 000 entries pruned after one pass: the kept entries move in chunks of at most 256, bit for bit"""
    model, hd, rec, hdr, vals = mined("shared", np.float32, n=48)
    flat = model.flatten()
    k = 3000
    idx = np.arange(k) % len(rec)
    ids = Q.ids_of_records(rec[idx], -1)
    ids[:, 1] = np.arange(k)
    ids[: k // 10, 0] = 1
    q, ref = Q.QP(hd, k), Q.QPRef(flat, k)
    assert q.add(hd, hdr[idx], vals[idx], ids=ids) == k
    ref.add(hdr[idx], vals[idx], ids)
    q.one(seed=2)
    ref.one(seed=2)
    same_state(q, ref)
    keep = ref.sv if not all(ref.sv) else [1 if ref.a[i] > 0 else 0 for i in range(k)]
    kept = [i for i in range(k) if keep[i]]
    first = next((j for j, i in enumerate(kept) if i != j), len(kept))
    assert len(kept) - first > 2 * 256, (len(kept), first)
    assert q.prune() == ref.prune()
    same_entries(q, ref)
    same_state(q, ref)
    hd.close()


def build_pair(name="person", dtype=np.float32, n=48, groups=False):
    model, hd, rec, hdr, vals = mined(name, dtype, n=n)
    flat = model.flatten()
    npos = n // 4
    ids = np.r_[Q.ids_of_records(rec[:npos], 1), Q.ids_of_records(rec[npos:], -1)]
    kw = {}
    if groups:      # negatives in groups of three whose first step saturates the group: the paired update through idI
        ids[npos:, 1:] = 0
        ids[npos:, 1] = np.arange(n - npos) // 3
        vals = vals * np.asarray(0.25, vals.dtype)
        kw = {"wreg": np.ones(E.vector_offsets(flat)[2])}   # no root-bias weighting: d stays below b
    q = Q.QP(hd, 2 * n, **kw)
    ref = Q.QPRef(flat, 2 * n, **kw)
    q.add(hd, hdr, vals, ids=ids)
    ref.add(hdr, vals, ids)
    return hd, q, ref, npos


@pytest.mark.parametrize("groups", [False, True])
def test_one_with_explicit_orders(groups):
    hd, q, ref, npos = build_pair(groups=groups)
    q.fix(); ref.fix()
    rng = np.random.default_rng(5)
    branches = []
    for t in range(4):
        nsv = sum(ref.sv)
        order = rng.permutation(nsv).astype(np.int32)
        q.one(order=order)
        ref.one(order=order)
        branches += ref.branches
        same_state(q, ref)
    assert "plain" in branches
    if groups:
        assert "pair" in branches
    hd.close()


def test_opt_seeded_and_prune_and_repeat():
    runs = []
    for rep in range(2):
        hd, q, ref, npos = build_pair(groups=True)
        q.fix(); ref.fix()
        for it in (1, 2):
            s = q.opt(tol=0.05, iter=1, seed=3 + it)
            ref.opt(tol=0.05, iter=1, seed=3 + it)
            same_state(q, ref)
            assert s["passes"] == 1
        n = q.prune()
        assert n == ref.prune()
        same_entries(q, ref)
        same_state(q, ref)
        s = q.opt(tol=0.05, iter=200, seed=11)
        ref.opt(tol=0.05, iter=200, seed=11)
        same_state(q, ref)
        assert s["converged"] and s["lb_dropped"] == 0 and 1 - s["lb"] / s["ub"] < 0.05
        assert q.scores().tobytes() == ref.scores().tobytes()
        assert q.weights().tobytes() == ref.weights().tobytes()
        runs.append(q.state(arrays=True)["w"].tobytes())
        hd.close()
    assert runs[0] == runs[1]


def test_qp_outlives_handle_and_refusals():
    model, hd, rec, hdr, vals = mined("shared", np.float32, n=16)
    q = Q.QP(hd, 8)
    with pytest.raises(PbdError):      # empty cache
        q.opt()
    with pytest.raises(PbdError):
        q.one()
    q.add(hd, hdr, vals, rec, label=1)
    hd.close()
    s = q.opt(tol=0.05, iter=50)
    assert s["n"] == 8 and np.all(np.isfinite(q.weights()))
    other = detector.Handle(M.synthetic_person_model(thresh=-100.0), device=0)
    with pytest.raises(PbdError):      # layout mismatch
        q.add(other, np.zeros((1, other.example_stride()[0]), np.int32), np.zeros((1, other.example_stride()[1]), np.float32),
              ids=np.ones((1, 5), np.int32))
    with pytest.raises(PbdError):
        q.opt(tol=float("nan"))
    with pytest.raises(PbdError):
        Q.QP(other, 0)
    with pytest.raises(PbdError):
        Q.QP(other, 4, C=float("nan"))
    other.close()


E2E = {"tiny": (lambda: M.synthetic_tiny_model(thresh=-1.0), (72, 96), [20, 16, 60, 56], 0.3),
       "person": (lambda: M.synthetic_person_model(thresh=-100.0), (120, 160), [0, 0, 159, 119], 0.0)}


@pytest.mark.parametrize("name", sorted(E2E))
def test_end_to_end_round(name):
    """latent positives + hard negatives -> add_device, fix, prune, opt -> weights -> Model.from_vector -> a new handle that
    detects; w . x of every positive's example (the records' feature vectors, which do not depend on w) with the trained vector
    equals scores() within the rounding bound, and the gap closed"""
    import torch
    make, (rows, cols), box, overlap = E2E[name]
    model = make()
    flat = model.flatten()
    det = detector.PartsBasedDetector(max_batch=4)
    det.distributeModel(model)
    frames = [synth.synthetic_frame(40 + k, rows, cols) for k in range(4)]
    boxes = [[box] * flat.max_parts for _ in frames]
    cands, found = det.detectLatent(frames, boxes, overlap)
    assert found.all()
    q = det.qp(256)
    hd = det.hd
    pos_rec = hd.pack_candidates(cands)
    hw, vw = hd.example_stride()
    st = hd.stride

    def push(rec, label, id_base):
        pay = torch.zeros(1 + len(rec) * st, dtype=torch.int32, device="cuda")
        pay[0] = len(rec)
        pay[1:] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
        dh = torch.zeros(len(rec) * hw, dtype=torch.int32, device="cuda")
        dv = torch.zeros(len(rec) * vw, dtype=torch.float32, device="cuda")
        hd.examples_device(pay.data_ptr(), len(rec), 0, dh.data_ptr(), dv.data_ptr())
        q.add_device(hd, pay.data_ptr(), len(rec), dh.data_ptr(), dv.data_ptr(), label, id_base)

    pos_hdr, pos_vals = hd.examples(pos_rec)     # of the latent result (the detect calls below replace it)
    push(pos_rec, 1, 0)
    q.fix()
    negs = [synth.synthetic_frame(90 + k, rows, cols, kind="noise") for k in range(2)]
    neg_rec = records(hd, negs)
    assert len(neg_rec) > 10
    push(neg_rec[:200], -1, 100)
    n0 = q.state()["n"]
    q.prune()
    s = q.opt(tol=0.05, iter=500, seed=1)
    assert s["converged"] and 1 - s["lb"] / s["ub"] < 0.05 and s["n"] <= n0
    w = q.weights()
    new_model = model.from_vector(w.astype(np.float32))
    det2 = detector.PartsBasedDetector(max_batch=4)
    det2.distributeModel(new_model)
    assert det2.modelVector().tobytes() == w.astype(np.float32).tobytes()   # the trained vector is the new handle's
    det2.detect(frames[0])                      # and it detects
    got = q.scores()
    want = E.dot(pos_hdr, pos_vals, w)
    bound = 1e-6 * E.abs_dot(pos_hdr, pos_vals, w) + 1e-9
    assert len(got) == len(pos_rec) and np.all(np.abs(got - want) <= bound)
