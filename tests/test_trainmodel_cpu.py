"""trainmodel_ref (partsbaseddetector_amd/trainmodel.py) on the case of tests/trainmodel_cases.py: the clustering finds the built
groups, the anchors follow from them, build_model gives the expected tree, the fixed-type pass places every positive in its
types, a type without a usable positive is refused, and a run resumed from idx= / part_models= equals the full run."""
import numpy as np
import pytest

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import train as T
from partsbaseddetector_amd import trainmodel as TM

import trainmodel_cases as TC


@pytest.fixture(scope="module")
def run():
    return TC.ref_run()


def test_clusters_are_the_built_groups(run):
    _, info = run
    g = TC.groups()
    for p in range(3):
        assert np.array_equal(info["idx"][p], g[p]) or np.array_equal(info["idx"][p], 1 - g[p]), p
    assert info["idx"].dtype == np.int32 and info["def"].shape == (3, TC.NPOS, 2)
    assert np.array_equal(info["cluster"]["counts"][:, :2], np.full((3, 2), 4))
    # the label order is the rules': type 0 is the group of the picked trial's first starting point that kept members
    again = TM.cluster_parts_ref(info["def"], [-1, 0, 1], TC.K, TC.TRIALS, 1000, TC.SEED)
    assert np.array_equal(again["idx"], info["idx"])


def test_anchors_follow_the_groups(run):
    _, info = run
    g = TC.groups()
    assert not info["anchors"][0].any()
    for p in (1, 2):
        for n in range(TC.NPOS):                      # 20 pixels = 5 cells to the right (group 0) or below (group 1)
            assert tuple(info["anchors"][p, info["idx"][p, n]]) == ((5, 0) if g[p, n] == 0 else (0, 5)), (p, n)
    assert np.array_equal(info["anchors"], TM.anchors_of(info["centres"]))
    assert np.array_equal(info["centres"].view(np.uint64), TM.centres_of(info["def"], [-1, 0, 1], info["idx"], TC.K).view(np.uint64))


def test_built_model_structure(run):
    _, info = run
    m = info["built"]
    m.validate()
    assert m.parentid == [[-1, 0, 1]] and m.filterid == [[[0, 1], [2, 3], [4, 5]]] and m.defid == [[[], [0, 1], [2, 3]]]
    assert m.biasid == [[[0], [1, 3, 2, 4], [5, 7, 6, 8]]] and m.biasw == [0.0] * 9
    assert m.defw == [[0.01, 0.0, 0.01, 0.0]] * 4 and (m.sbin, m.interval, m.thresh) == (TC.SBIN, 10, 0.0)
    assert m.anchors == [tuple(int(v) for v in info["anchors"][p, k]) for p in (1, 2) for k in range(2)]
    for p in range(3):
        pm = info["part_models"][p]
        assert pm.ncomponents() == 2 and all(f.shape == (5, 160) for f in pm.filtersw)
        for k in range(2):
            assert np.array_equal(m.filtersw[2 * p + k], pm.filtersw[k]) and pm.filtersw[k].any()
            assert info["part_info"][p][k]["numpositives"] == [4] and info["part_info"][p][k]["skipped"] == []
    assert len(m.to_vector()) == 9 + 16 + 6 * 5 * 5 * 32


def test_fixed_type_pass_places_every_positive_in_its_types(run):
    model, info = run
    assert info["final1"]["notfound"] == [] and info["final1"]["skipped"] == [] and info["final1"]["numpositives"] == [TC.NPOS]
    assert info["final"]["notfound"] == [] and info["final"]["skipped"] == [] and info["final"]["numpositives"] == [TC.NPOS]
    pos, _, kw = TC.case()
    for n, p in enumerate(pos):
        crop, bx = T.croppos(T._frame(p["im"]), T.part_boxes(p))
        got = E.latent_search(info["built"], crop, bx, kw["overlap"], info["idx"][:, n], np.float32, walk="argmax")
        assert got["found"] and [m for _, _, m in got["placement"]] == info["idx"][:, n].tolist(), n
    assert np.float32(model.thresh) == np.float32(info["final"]["thresh"])
    assert model.to_vector().shape == info["model1"].to_vector().shape and model.to_vector().any()


def test_a_type_without_a_usable_positive_is_refused(run):
    _, info = run
    pos, neg, kw = TC.case()
    idx = info["idx"].copy()
    idx[2] = 0
    with pytest.raises(ValueError, match="part 2 type 1"):
        TM.trainmodel_ref(pos, neg, idx=idx, **kw)
    small = [dict(p, boxes=p["boxes"].copy()) for p in pos]
    for n, p in enumerate(small):
        if info["idx"][0, n] == 0:
            p["boxes"][0, 2] -= 1                     # 19 x 20 pixels: below minsize = (5 * 4)^2
    with pytest.raises(ValueError, match="part 0 type 0"):
        TM.trainmodel_ref(small, neg, idx=info["idx"], **kw)


def test_resume_equals_the_full_run(run):
    model, info = run
    pos, neg, kw = TC.case()
    again, info2 = TM.trainmodel_ref(pos, neg, idx=info["idx"], part_models=info["part_models"], **kw)
    assert again.to_vector().tobytes() == model.to_vector().tobytes()
    assert np.float32(again.thresh).tobytes() == np.float32(model.thresh).tobytes()
    assert info2["model1"].to_vector().tobytes() == info["model1"].to_vector().tobytes()
    assert info2["cluster"] is None and info2["part_info"] is None
    assert np.array_equal(info2["anchors"], info["anchors"]) and info2["final"] == info["final"] and info2["final1"] == info["final1"]
