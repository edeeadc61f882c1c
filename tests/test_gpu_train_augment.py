"""Training on device-resident positives and with augmentation: train() on device tensors against train()
on the same host arrays (the warp case and the latent case of tests/train_cases.py), trainmodel(augment=...) against
trainmodel_ref(augment=...) bit for bit on the case tests/test_augment_cpu.py checked on the CPU, and trainmodel(augment=None)
against the unchanged yardstick run of tests/trainmodel_cases.py."""
import numpy as np
import pytest

from partsbaseddetector_amd import train as T
from partsbaseddetector_amd import trainmodel as TM

import augment_cases as AC
import train_cases
import trainmodel_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def same_info(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in ("iterations", "batches"):
            assert len(got[k]) == len(want[k])
            for a, b in zip(got[k], want[k]):
                same_info(a, b)
        elif isinstance(want[k], float):
            assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])


def same_model(got, want):
    assert got.to_vector(np.float32).tobytes() == want.to_vector(np.float32).tobytes()
    assert np.float32(got.thresh).tobytes() == np.float32(want.thresh).tobytes()
    assert (got.filterid, got.biasid, got.defid, got.parentid) == (want.filterid, want.biasid, want.defid, want.parentid)
    assert [tuple(a) for a in got.anchors] == [tuple(a) for a in want.anchors] and (got.interval, got.sbin) == (want.interval, want.sbin)


def on_device(pos):
    """the positives with their images on the device: contiguous tensors, and every second one a view of a larger device image"""
    import torch
    out = []
    for n, p in enumerate(pos):
        im = p["im"]
        if n % 2:
            big = np.full((im.shape[0] + 9, im.shape[1] + 14) + im.shape[2:], 50, im.dtype)
            big[4:4 + im.shape[0], 6:6 + im.shape[1]] = im
            t = torch.from_numpy(big).cuda()[4:4 + im.shape[0], 6:6 + im.shape[1]]
            assert not t.is_contiguous()
        else:
            t = torch.from_numpy(np.array(im)).cuda()
        out.append(dict(p, im=t))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,warp", [("warp_case", 1), ("latent_case", 0)])
def test_train_on_device_tensors_equals_train_on_host_arrays(name, warp):
    model, pos, neg, kw = getattr(train_cases, name)()
    want_model, want = T.train(model, pos, neg, warp, dtype=np.float32, **kw)
    dpos = on_device(pos)
    got_model, got = T.train(model, dpos, neg, warp, dtype=np.float32, **kw)
    same_info(got, want)
    same_model(got_model, want_model)
    assert sum(want["numpositives"]) >= 4 and want["lb"] > 0
    host = T.host_positives(dpos)                                  # what the yardsticks work on
    assert all(isinstance(h["im"], np.ndarray) and np.array_equal(h["im"], p["im"]) for h, p in zip(host, pos))
    with pytest.raises(ValueError):
        T.train(model, [dpos[0]] + list(pos[1:]), neg, warp, dtype=np.float32, **kw)


@pytest.fixture(scope="module")
def augmented_runs():
    pos, neg, kw, aug = AC.train_case()
    return TM.trainmodel(pos, neg, dtype=np.float32, augment=aug, **kw), AC.ref_run()


def test_trainmodel_augment_equals_the_yardstick(augmented_runs):
    (model, got), (ref, want) = augmented_runs
    assert got["augment"] == want["augment"] == {"degrees": [15.0], "mirror": [0, 1, 2], "copies": 4, "total": 16}
    assert got["def"].tobytes() == want["def"].tobytes()
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["anchors"], want["anchors"])
    for p in range(3):
        same_model(got["part_models"][p], want["part_models"][p])
        for k in range(2):
            same_info(got["part_info"][p][k], want["part_info"][p][k])
    same_model(got["built"], want["built"])
    same_model(got["model1"], want["model1"])
    same_info(got["final1"], want["final1"])
    same_model(model, ref)
    same_info(got["final"], want["final"])
    assert sum(got["final"]["numpositives"]) == 12 and got["final"]["notfound"] == []


def test_trainmodel_without_augment_is_unchanged():
    pos, neg, kw = TC.case()
    model, got = TM.trainmodel(pos, neg, dtype=np.float32, augment=None, **kw)
    ref, want = TC.ref_run()
    assert "augment" not in got and "augment" not in want
    same_model(model, ref)
    same_model(got["model1"], want["model1"])
    same_info(got["final1"], want["final1"])
    same_info(got["final"], want["final"])
    assert np.array_equal(got["idx"], want["idx"])
