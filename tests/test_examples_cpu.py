"""CPU tests of the training-example yardstick (partsbaseddetector_amd/examples.py): the model vector, the walk and gather of
an example, and the score identity w . x, against a brute-force enumeration of every placement of small models."""
import itertools

import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import synthetic_frame


def _small_models():
    # 3 parts x 2 mixtures (linear deformations), and a 2-part model of 3 mixtures with 3x3 filters
    return [M.synthetic_tiny_model(), M.synthetic_model(seed=5, pa=[0, 1], nmix=3, ksize=3, linear_def=True, interval=3)]


def _brute_force(flat, c, resp):
    """best[(p, mixture)] (H, W): the best score of part p's subtree with p at every cell and mixture, by enumerating every
    child placement (no distance transform); rootv: max over root mixtures + the root bias"""
    _, H, W = resp.shape
    p0 = int(flat.part_offset[c])
    np_c = int(flat.part_offset[c + 1]) - p0
    ys, xs = np.mgrid[0:H, 0:W]
    best = {}
    for p in range(np_c - 1, -1, -1):
        gp = p0 + p
        K = int(flat.mix_offset[gp + 1] - flat.mix_offset[gp])
        for m in range(K):
            v = resp[int(flat.filterid[flat.mix_offset[gp] + m])].astype(np.float64)
            for ch in range(p + 1, np_c):
                if int(flat.parentid[p0 + ch]) != p:
                    continue
                gc = p0 + ch
                msg = np.full((H, W), -np.inf)
                for mm in range(int(flat.mix_offset[gc + 1] - flat.mix_offset[gc])):
                    gm = int(flat.mix_offset[gc]) + mm
                    d = int(flat.defid[gm])
                    w = [float(t) for t in flat.defw[d]]
                    ax, ay = (int(t) for t in flat.anchors[d])
                    b = float(flat.biasw[int(flat.biasid[gm]) + m])
                    for py, px in itertools.product(range(H), range(W)):
                        dx, dy = px + ax - xs, py + ay - ys
                        cand = best[(ch, mm)] + b - (w[0] * dx * dx + w[1] * dx + w[2] * dy * dy + w[3] * dy)
                        msg[py, px] = max(msg[py, px], cand.max())
                v = v + msg
            best[(p, m)] = v
    K0 = int(flat.mix_offset[p0 + 1] - flat.mix_offset[p0])
    root = np.max([best[(0, m)] for m in range(K0)], axis=0) + float(flat.biasw[flat.biasid[flat.mix_offset[p0]]])
    return root, best


def _true_walk(flat, c, best, x, y):
    """the arg-max placement from the root at (x, y), found by enumeration (the reference's composed pointers need not give it)"""
    p0 = int(flat.part_offset[c])
    np_c = int(flat.part_offset[c + 1]) - p0
    H, W = best[(0, 0)].shape
    ys, xs = np.mgrid[0:H, 0:W]
    K0 = int(flat.mix_offset[p0 + 1] - flat.mix_offset[p0])
    out = [(x, y, int(np.argmax([best[(0, m)][y, x] for m in range(K0)])))]
    for p in range(1, np_c):
        px, py, pm = out[int(flat.parentid[p0 + p])]
        gc = p0 + p
        top = None
        for mm in range(int(flat.mix_offset[gc + 1] - flat.mix_offset[gc])):
            gm = int(flat.mix_offset[gc]) + mm
            d = int(flat.defid[gm])
            w = [float(t) for t in flat.defw[d]]
            dx, dy = px + int(flat.anchors[d][0]) - xs, py + int(flat.anchors[d][1]) - ys
            cand = best[(p, mm)] + float(flat.biasw[int(flat.biasid[gm]) + pm]) - (w[0] * dx * dx + w[1] * dx + w[2] * dy * dy + w[3] * dy)
            i = int(np.argmax(cand))
            if top is None or cand.flat[i] > top[0]:
                top = (cand.flat[i], (i % W, i // W, mm))
        out.append(top[1])
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_walked_examples_reproduce_brute_force_scores(oracle, which):
    """On random feature maps: the oracle's DP equals the brute-force best placement, and every root's example (walked through
    the oracle's maps) scores w . x = its placement's score; where the placement is the true arg-max, w . x = rootv."""
    model = _small_models()[which]
    flat = model.flatten()
    w = E.model_vector(flat, np.float32)
    rng = np.random.default_rng(7 + which)
    H, Wd = 6, 8
    feat = rng.standard_normal((H, Wd * 32)).astype(np.float32)
    resp = oracle.responses(flat, feat)
    Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, 0, resp)
    brute, best = _brute_force(flat, 0, resp)
    np.testing.assert_allclose(rootv.astype(np.float64), brute, rtol=0, atol=1e-4)
    exact = 0
    for y, x in itertools.product(range(H), range(Wd)):
        pl = E.walk(flat, 0, x, y, Ix, Iy, Ik, rooti)
        hdr, vals = E.example(flat, feat, 0, pl, 0, np.float32)
        got = E.dot(hdr, vals, w)[0]
        bound = E.rounding_bound(flat, hdr, vals, w)[0]
        ps = E.placement_score(flat, resp, 0, pl)
        assert abs(got - ps) <= bound + 1e-6, (x, y, got, ps, bound)
        assert got <= float(rootv[y, x]) + bound + 1e-5
        if abs(ps - brute[y, x]) <= 1e-5:
            exact += 1
            assert abs(got - float(rootv[y, x])) <= bound + 1e-5
        # the example of the true arg-max placement scores exactly the DP's value
        hdr, vals = E.example(flat, feat, 0, _true_walk(flat, 0, best, x, y), 0, np.float32)
        assert abs(E.dot(hdr, vals, w)[0] - float(rootv[y, x])) <= E.rounding_bound(flat, hdr, vals, w)[0] + 1e-5
    assert exact >= 1


def test_identity_on_every_oracle_record(oracle):
    """The w . x identity on every record the oracle detects in a frame (tiny model; windows crossing the map border)"""
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    im = synthetic_frame(5, 72, 96)
    recs = oracle.detect(flat, im)
    assert len(recs) > 20
    fm = E.FrameMaps(flat, im)
    w = E.model_vector(flat)
    border = 0
    for r in recs:
        pl = fm.placement(r["level"], r["component"], r["root_x"], r["root_y"])
        hdr, vals = E.example(flat, fm.feats[r["level"]], r["component"], pl, 0)
        H, Wc = fm.feats[r["level"]].shape[0], fm.feats[r["level"]].shape[1] // 32
        border += any(x < 2 or y < 2 or x >= Wc - 2 or y >= H - 2 for x, y, _ in pl)
        got = E.dot(hdr, vals, w)[0]
        bound = E.rounding_bound(flat, hdr, vals, w)[0]
        ps = E.placement_score(flat, fm.resp(r["level"]), r["component"], pl)
        assert abs(got - ps) <= bound + 1e-6
        assert got <= r["score"] + bound + 1e-5
    assert border > 0


def test_window_border_values():
    feat = np.arange(2 * 3 * 32, dtype=np.float32).reshape(2, 3 * 32)
    win = E.window(feat, 0, 0, 3).reshape(3, 3, 32)
    assert np.all(win[0, :, :31] == 0) and np.all(win[0, :, 31] == 1) and np.all(win[:, 0, 31] == 1)
    assert np.array_equal(win[1, 1], feat[0, :32]) and np.array_equal(win[2, 2], feat[1, 32:64])


def test_header_layout_and_densify():
    model = M.synthetic_tiny_model()
    flat = model.flatten()
    feat = np.ones((4, 4 * 32), np.float32)
    pl = [(1, 1, 0), (2, 1, 1), (0, 3, 0)]
    hdr, vals = E.example(flat, feat, 0, pl, 7)
    hw, vw = E.strides(flat)
    assert hdr.shape == (hw,) and vals.shape == (vw,)
    assert hdr[0] == 7 and hdr[1] == 0 and hdr[2] == 3 * 3 - 1 and hdr[3] == 1 + 800 + 2 * (5 + 800)
    dbase, fbase, n = E.vector_offsets(flat)
    assert hdr[4:6].tolist() == [int(flat.biasid[0]), 1]
    assert hdr[6:8].tolist() == [fbase + int(flat.filter_offset[flat.filterid[0]]), 800]
    # part 1 (mixture 1, parent mixture 0): bias(1)[0], deformation of mixture 1
    gm = int(flat.mix_offset[1]) + 1
    assert hdr[8:12].tolist() == [int(flat.biasid[gm]), 1, dbase + 4 * int(flat.defid[gm]), 4]
    d = int(flat.defid[gm])
    dx, dy = 1 + int(flat.anchors[d][0]) - 2, 1 + int(flat.anchors[d][1]) - 1
    assert vals[801:806].tolist() == [1, -dx * dx, -dx, -dy * dy, -dy]
    dense = E.densify(hdr, vals, n)
    w = E.model_vector(flat).astype(np.float64)
    assert abs(float(dense[0] @ w) - E.dot(hdr, vals, w)[0]) < 1e-9


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_vector_round_trips_bit_for_bit(dtype):
    for model in [M.synthetic_tiny_model(), M.synthetic_face_model(nparts=5), _small_models()[1]]:
        w = model.to_vector(dtype)
        flat = model.flatten()
        dbase, fbase, n = E.vector_offsets(flat)
        assert len(w) == n == len(flat.biasw) + 4 * len(flat.defw) + len(flat.filters_f32)
        back = model.from_vector(w)
        w2 = back.to_vector(dtype)
        assert w2.dtype == np.dtype(dtype) and w2.tobytes() == w.tobytes()
        f2 = back.flatten()
        assert f2.biasw.tobytes() == flat.biasw.tobytes() and f2.defw.tobytes() == flat.defw.tobytes()
        filt = flat.filters_f32 if dtype == np.float32 else flat.filters_f64
        assert (f2.filters_f32 if dtype == np.float32 else f2.filters_f64).tobytes() == filt.tobytes()


def test_from_vector_rejects_a_wrong_length():
    model = M.synthetic_tiny_model()
    with pytest.raises(ValueError):
        model.from_vector(np.zeros(5, np.float32))
