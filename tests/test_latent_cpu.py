"""CPU tests of the latent-positive yardstick (partsbaseddetector_amd/examples.py latent_search): the winner is the best placement
whose every part passes the overlap test, against a brute-force enumeration of every placement; fixed mixtures; boxes off the
image."""
import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import synthetic_frame

from test_examples_cpu import _brute_force, _small_models


def _boxes_of(oracle, model, im):
    """the part boxes (inclusive corners) of the oracle's best detection of im"""
    recs = oracle.detect(model.flatten(), im)
    best = max(recs, key=lambda r: r["score"])
    return [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best["parts"]]


@pytest.mark.parametrize("which", [0, 1])
def test_latent_winner_is_the_best_passing_placement(oracle, which):
    model = _small_models()[which]
    model.thresh = -100.0
    im = synthetic_frame(11 + which, 40, 56)
    boxes = _boxes_of(oracle, model, im)
    for overlap, mixtures in ((0.3, None), (0.5, None), (0.3, [1] + [-1] * (len(boxes) - 1))):
        got = E.latent_search(model, im, boxes, overlap, mixtures)
        uflat = E.unique_model(model).flatten()
        feats, scales = oracle.features_pyramid(uflat, im)
        brute = -np.inf
        for lvl, feat in enumerate(feats):
            resp = E.mask_responses(uflat, oracle.responses(uflat, feat), scales[lvl], boxes, overlap, mixtures)
            root, _ = _brute_force(uflat, 0, resp)
            brute = max(brute, float(root.max()))
        assert got["found"] == (brute > -5e9)
        assert abs(got["score"] - brute) <= 1e-4 * max(1.0, abs(brute))
        if got["found"]:
            # the root sits where the dynamic program put it, so it passes; the children are walked with the reference's
            # pointer composition, which can place one off its arg-max, so they are not asserted here
            x, y, w, h = got["parts"][0]
            assert E.overlap_passes((np.int64(x), np.int64(y), np.int64(x + w), np.int64(y + h)), boxes[0], overlap)
            if mixtures is not None:
                assert got["placement"][0][2] == 1


def test_boxes_off_the_image_find_nothing(oracle):
    model = M.synthetic_tiny_model()
    got = E.latent_search(model, synthetic_frame(3, 40, 56), [(5000, 5000, 5040, 5040)] * 3, 0.1)
    assert not got["found"] and got["score"] < -5e9


def test_unique_model_copies_shared_filters():
    m = M.synthetic_face_model(nparts=4, ncomponents=2)
    u = E.unique_model(m)
    fu = u.flatten()
    assert fu.nfilters == int(fu.mix_offset[-1]) and list(fu.filterid) == list(range(fu.nfilters))
    f = m.flatten()
    for gm in range(fu.nfilters):
        assert np.array_equal(u.filtersw[gm], m.filtersw[int(f.filterid[gm])])
