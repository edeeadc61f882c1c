"""Training on the device: pbd_qp_clear and pbd_qp_add_loss_device bit for bit against QPRef, and train() against train_ref()
(partsbaseddetector_amd/train.py) on the cases of tests/train_cases.py -- the model vector and the threshold bit for bit, the
info field for field -- for float and double, and a second iteration (the clear path)."""
import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd import train as T
from partsbaseddetector_amd.detector import PbdError

import train_cases as TC
from test_gpu_qp import device_add, mined, same_entries, same_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def test_clear_then_readd_equals_a_fresh_qp():
    model, hd, rec, hdr, vals = mined("shared", np.float32, n=40)
    try:
        flat = model.flatten()
        q, fresh, ref = Q.QP(hd, 48), Q.QP(hd, 48), Q.QPRef(flat, 48)
        assert q.add(hd, hdr[::-1], vals[::-1], rec[::-1], label=-1, id_base=3) == 40
        q.fix()
        q.opt(0.05, 4, 1)
        q.clear()
        st = q.state()
        assert (st["n"], st["nsv"], st["nfix"], st["l"], st["loss"]) == (0, 0, 0, 0.0, 0.0)
        assert st["lb"] != st["lb"] and st["ub"] != st["ub"]
        hw, vw = hd.example_stride()
        for qq in (q, fresh):
            assert qq.add(hd, hdr[:10], vals[:10], rec[:10], label=1, id_base=7) == 10
            assert device_add(qq, hd, rec[10:], hw, vw, np.float32, -1, 7) == 30
        ref.add(hdr[:10], vals[:10], Q.ids_of_records(rec[:10], 1, 7))
        ref.add(hdr[10:], vals[10:], Q.ids_of_records(rec[10:], -1, 7))
        same_entries(q, ref)
        same_entries(fresh, ref)
        ref.fix()
        ref.opt(0.05, 6, 2)
        for qq in (q, fresh):
            qq.fix()
            qq.opt(0.05, 6, 2)
            same_state(qq, ref)
    finally:
        hd.close()


@pytest.fixture(scope="module")
def ready():
    """a QP with an upper bound, its yardstick and its handle"""
    model, hd, rec, hdr, vals = mined("shared", np.float32, n=12)
    q, ref = Q.QP(hd, 16), Q.QPRef(model.flatten(), 16)
    with pytest.raises(PbdError) as e:                      # no opt / one yet: ub is NaN
        q.add_loss_device(0, 0, -1)
    assert e.value.code in (-1, -5)
    q.add(hd, hdr, vals, rec, label=1)
    ref.add(hdr, vals, Q.ids_of_records(rec, 1, 0))
    yield q, ref, hd
    hd.close()


def test_add_loss_refused_before_the_first_opt(ready):
    import torch
    _, _, hd = ready
    q = Q.QP(hd, 4)
    pay = torch.zeros(1 + hd.stride, dtype=torch.int32, device="cuda")
    with pytest.raises(PbdError) as e:
        q.add_loss_device(pay.data_ptr(), 1, -1)
    assert e.value.code == -5
    with pytest.raises(PbdError) as e:
        q.add_loss_device(pay.data_ptr(), -1, -1)
    assert e.value.code == -1


@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 5000])
def test_add_loss_device_bit_for_bit(ready, n):
    import torch
    q, ref, hd = ready
    if ref.ub != ref.ub:
        q.fix(); ref.fix()
        q.one(seed=4); ref.one(seed=4)
    rng = np.random.default_rng(100 + n)
    s = (rng.standard_normal(n) * 1.5 - 1.0).astype(np.float32)
    if n > 3:
        s[1], s[2], s[3] = -1.0, np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(-2))
    rec = np.zeros((n, hd.stride), np.int32)
    rec[:, 5] = s.view(np.int32)
    cap = n + 2
    pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = n
    if n:
        pay[1:1 + rec.size] = torch.from_numpy(rec.ravel()).cuda()
    torch.cuda.synchronize()
    for label in (-1, 1):
        got = q.add_loss_device(pay.data_ptr(), cap, label)
        want = ref.add_loss(rec, label)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, label, got, want)
        assert np.float64(q.state()["ub"]).tobytes() == np.float64(ref.ub).tobytes()
    if n >= 1023:
        # word 0 above the capacity: only the records present count
        pay[0] = n + 1000
        torch.cuda.synchronize()
        got = q.add_loss_device(pay.data_ptr(), 1000, -1)
        assert np.float64(got).tobytes() == np.float64(ref.add_loss(rec[:1000], -1)).tobytes()
        pay[0] = -3
        torch.cuda.synchronize()
        assert q.add_loss_device(pay.data_ptr(), cap, -1) == 0.0 and ref.add_loss(rec[:0], -1) == 0.0


def same_info(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if k == "iterations":
            assert len(got[k]) == len(want[k])
            for a, b in zip(got[k], want[k]):
                same_info(a, b)
        elif k == "batches":
            assert len(got[k]) == len(want[k])
            for a, b in zip(got[k], want[k]):
                same_info(a, b)
        elif isinstance(want[k], float):
            assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])


def check_train(case, warp, dtype, **extra):
    model, pos, neg, kw = case()
    kw = dict(kw, **extra)
    want_model, want = T.train_ref(model, pos, neg, warp, dtype=dtype, **kw)
    got_model, got = T.train(model, pos, neg, warp, dtype=dtype, **kw)
    same_info(got, want)
    assert got_model.to_vector(dtype).tobytes() == want_model.to_vector(dtype).tobytes()
    assert np.float32(got_model.thresh).tobytes() == np.float32(want_model.thresh).tobytes()
    assert (got_model.interval, got_model.sbin) == (model.interval, model.sbin)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_train_latent_case_equals_train_ref(dtype):
    info = check_train(TC.latent_case, 0, dtype)
    assert {"opt+prune", "one"} <= {b["branch"] for b in info["batches"]} and info["lb"] > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_train_warp_case_equals_train_ref(dtype):
    info = check_train(TC.warp_case, 1, dtype)
    assert info["skipped"] == [3] and info["lb"] > 0


def test_train_second_iteration_equals_train_ref():
    info = check_train(TC.latent_case, 0, np.float32, iters=2)
    assert len(info["iterations"]) == 2
