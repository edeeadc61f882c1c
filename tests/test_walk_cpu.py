"""CPU tests of the arg-max walk's yardstick (partsbaseddetector_amd/examples.py raw_maps, compose, walk(argmax=True)):
raw_maps pinned bit for bit on oracle.dp_min through the reference's own composition, and the arg-max placement's score equal
to the dynamic program's value -- and to a brute-force maximum over every placement -- where the composed walk's is not."""
import itertools

import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import synthetic_frame

from test_examples_cpu import _brute_force, _small_models


def shared_model():
    """tiny model whose part 2 uses part 1's filters (one filter id twice inside a component)"""
    m = M.synthetic_tiny_model(thresh=-1.0)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def mixed_count_model():
    """parts that differ in mixture count: the root 2, part 1 one (reduceMax copies), part 2 three"""
    m = M.synthetic_model(seed=9, pa=[0, 1, 1], nmix=3, ksize=3, linear_def=True, interval=3)
    keep = [2, 1, 3]
    for p, k in enumerate(keep):
        m.filterid[0][p] = m.filterid[0][p][:k]
        m.defid[0][p] = m.defid[0][p][:k]
        m.biasid[0][p] = m.biasid[0][p][:k]
    m.validate()
    return m


MODELS = {
    "tiny": lambda: M.synthetic_tiny_model(thresh=-1.0),
    "shared": shared_model,
    "three_components": lambda: M.synthetic_face_model(nparts=7, ncomponents=3, thresh=-100.0),
    "mixed_counts": mixed_count_model,
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_raw_maps_composed_equal_dp_min_bit_for_bit(oracle, name, dtype):
    """raw_maps + the reference's composition == oracle.dp_min (Ix, Iy, Ik, rootv, rooti) on the feature maps of a 72 x 96
    frame: the first, a middle and the last level, every component"""
    flat = MODELS[name]().flatten()
    feats, _ = oracle.features_pyramid(flat, synthetic_frame(5, 72, 96), dtype)
    for lvl in sorted({0, len(feats) // 2, len(feats) - 1}):
        resp = oracle.responses(flat, feats[lvl])
        for c in range(flat.ncomponents):
            Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, c, resp)
            IxRaw, IyRaw, Ik2, rootv2, rooti2 = E.raw_maps(flat, c, resp)
            assert rootv2.dtype == rootv.dtype and rootv2.tobytes() == rootv.tobytes(), (lvl, c)
            assert np.array_equal(rooti2, rooti)
            p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
            slots = [int(flat.ptr_slot[gp]) + pm for gp in range(p0 + 1, p1)
                     for pm in range(int(flat.mix_offset[p0 + int(flat.parentid[gp]) + 1] - flat.mix_offset[p0 + int(flat.parentid[gp])]))]
            cIx, cIy = E.compose(flat, c, IxRaw, IyRaw, Ik2)
            for s in slots:
                assert np.array_equal(Ik2[s], Ik[s]), (lvl, c, s)
                assert np.array_equal(cIx[s], Ix[s]), (lvl, c, s)
                assert np.array_equal(cIy[s], Iy[s]), (lvl, c, s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_argmax_placement_scores_rootv_at_every_root(oracle, dtype):
    """for every root of two small maps the arg-max placement's score is rootv within the rounding bound; the composed walk's is
    not, at one root at least"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    w = E.model_vector(flat, dtype)
    feats, _ = oracle.features_pyramid(flat, synthetic_frame(5, 72, 96), dtype)
    differs = 0
    for feat in (feats[0], feats[-1]):
        resp = oracle.responses(flat, feat)
        Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, 0, resp)
        IxRaw, IyRaw, Ik2, _, _ = E.raw_maps(flat, 0, resp)
        H, Wd = rootv.shape
        for y, x in itertools.product(range(H), range(Wd)):
            pl = E.walk(flat, 0, x, y, IxRaw, IyRaw, Ik2, rooti, argmax=True)
            hdr, vals = E.example(flat, feat, 0, pl, 0, dtype)
            bound = E.rounding_bound(flat, hdr, vals, w, dtype)[0]
            assert abs(E.placement_score(flat, resp, 0, pl) - float(rootv[y, x])) <= bound, (x, y)
            assert abs(E.dot(hdr, vals, w)[0] - float(rootv[y, x])) <= bound, (x, y)
            ref = E.walk(flat, 0, x, y, Ix, Iy, Ik, rooti)
            hdr, vals = E.example(flat, feat, 0, ref, 0, dtype)
            differs += abs(E.placement_score(flat, resp, 0, ref) - float(rootv[y, x])) > E.rounding_bound(flat, hdr, vals, w, dtype)[0]
    assert differs >= 1


@pytest.mark.parametrize("which", [0, 1])
def test_argmax_placement_is_the_brute_force_maximum(oracle, which):
    """on a map small enough to enumerate: the arg-max placement scores the maximum over all placements from that root"""
    flat = _small_models()[which].flatten()
    w = E.model_vector(flat, np.float32)
    rng = np.random.default_rng(7 + which)
    H, Wd = 6, 8
    feat = rng.standard_normal((H, Wd * 32)).astype(np.float32)
    resp = oracle.responses(flat, feat)
    Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, 0, resp)
    IxRaw, IyRaw, Ik2, rootv2, _ = E.raw_maps(flat, 0, resp)
    assert rootv2.tobytes() == rootv.tobytes()
    brute, _ = _brute_force(flat, 0, resp)
    differs = 0
    for y, x in itertools.product(range(H), range(Wd)):
        pl = E.walk(flat, 0, x, y, IxRaw, IyRaw, Ik2, rooti, argmax=True)
        hdr, vals = E.example(flat, feat, 0, pl, 0, np.float32)
        bound = E.rounding_bound(flat, hdr, vals, w)[0]
        assert abs(E.placement_score(flat, resp, 0, pl) - brute[y, x]) <= bound, (x, y)
        ref = E.walk(flat, 0, x, y, Ix, Iy, Ik, rooti)
        hdr, vals = E.example(flat, feat, 0, ref, 0, np.float32)
        differs += abs(E.placement_score(flat, resp, 0, ref) - brute[y, x]) > E.rounding_bound(flat, hdr, vals, w)[0]
    assert differs >= 1


def test_frame_maps_and_records_carry_the_mode(oracle):
    """FrameMaps(walk=), examples_of_records(walk=): every oracle record's arg-max example scores the record's score"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    im = synthetic_frame(5, 72, 96)
    recs = oracle.detect(flat, im)
    rec = np.zeros((len(recs), 8 + 4 * flat.max_parts), np.int32)
    for i, r in enumerate(recs):
        rec[i, :5] = (0, r["component"], r["level"], r["root_x"], r["root_y"])
    fm = E.FrameMaps(flat, im, walk="argmax")
    hdr, vals = E.examples_of_records(flat, [fm], rec)
    w = E.model_vector(flat)
    got, bound = E.dot(hdr, vals, w), E.rounding_bound(flat, hdr, vals, w)
    for i, r in enumerate(recs):
        assert abs(got[i] - r["score"]) <= bound[i] + abs(r["score"]) * 2.0 ** -24, i
    ref_h, ref_v = E.examples_of_records(flat, [fm], rec, walk="reference")
    assert not (np.array_equal(ref_h, hdr) and ref_v.tobytes() == vals.tobytes())
    want_h, want_v = E.examples_of_records(flat, [E.FrameMaps(flat, im)], rec)
    assert np.array_equal(ref_h, want_h) and ref_v.tobytes() == want_v.tobytes()
