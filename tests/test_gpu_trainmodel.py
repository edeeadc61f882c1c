"""trainmodel() on the device against trainmodel_ref() (partsbaseddetector_amd/trainmodel.py) on the case of
tests/trainmodel_cases.py, in float: the part types, the anchors, every part model, the model after each latent pass and the
threshold bit for bit, every info field, and the saved model file read back to the same detections.  T = double is covered for
the clustering (tests/test_gpu_cluster_parts.py) and for train() (tests/test_gpu_train.py)."""
import os

import numpy as np
import pytest

from partsbaseddetector_amd import load_model_file, synth
from partsbaseddetector_amd import trainmodel as TM
from partsbaseddetector_amd.detector import PartsBasedDetector
from partsbaseddetector_amd.modelfile import save_model_file

import trainmodel_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def runs():
    pos, neg, kw = TC.case()
    return TM.trainmodel(pos, neg, dtype=np.float32, **kw), TC.ref_run()


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


def test_clustering_equals_the_yardstick(runs):
    (_, got), (_, want) = runs
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["anchors"], want["anchors"])
    assert got["def"].tobytes() == want["def"].tobytes()
    assert np.array_equal(np.isnan(got["centres"]), np.isnan(want["centres"]))
    ok = ~np.isnan(want["centres"])
    assert got["centres"][ok].tobytes() == want["centres"][ok].tobytes()
    for k in ("counts", "iters_all", "info"):
        assert np.array_equal(got["cluster"][k], want["cluster"][k]), k
    assert got["cluster"]["sumdist_all"].tobytes() == want["cluster"]["sumdist_all"].tobytes()


def test_part_models_equal_the_yardstick(runs):
    (_, got), (_, want) = runs
    for p in range(3):
        same_model(got["part_models"][p], want["part_models"][p])
        for k in range(2):
            same_info(got["part_info"][p][k], want["part_info"][p][k])


def test_latent_passes_equal_the_yardstick(runs):
    (model, got), (ref, want) = runs
    same_model(got["built"], want["built"])
    same_model(got["model1"], want["model1"])
    same_info(got["final1"], want["final1"])
    same_model(model, ref)
    same_info(got["final"], want["final"])
    assert got["final"]["notfound"] == [] and got["final1"]["notfound"] == []


def test_saved_model_detects_the_same(runs, tmp_path):
    (model, _), _ = runs
    path = os.path.join(str(tmp_path), "trained.xml")
    save_model_file(model, path)
    back = load_model_file(path)
    im = synth.synthetic_frame(80, 72, 96)
    out = []
    for m in (model, back):
        m.thresh = -1.0
        det = PartsBasedDetector()
        det.distributeModel(m)
        try:
            out.append(det.detect(im))
        finally:
            det.hd.close()
    a, b = out
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert (x.level, x.component, tuple(x.root)) == (y.level, y.component, tuple(y.root))
        assert np.array_equal(x.parts, y.parts) and np.float32(x.score()) == np.float32(y.score())
