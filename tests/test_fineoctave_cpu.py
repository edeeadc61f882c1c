"""CPU tests of the fine octave's rule (partsbaseddetector_amd/fineoctave.py) against the oracle: off is
oracle.detect, the reference's levels keep their records, the fine levels hold records no other setting can produce, a planted
half-size object is found only with the octave on, a changed rule changes the records, and the plan arithmetic."""
import numpy as np
import pytest

from partsbaseddetector_amd import fineoctave as F
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import padding as P
from partsbaseddetector_amd import synthetic_frame

import fineoctave_cases as cases

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def model():
    return M.synthetic_tiny_model(thresh=-1.0)


@pytest.fixture(scope="module")
def frame():
    return synthetic_frame(5, 48, 64)


_runs = {}


def _run(model, frame, fine, dtype, **changed):
    key = (fine, np.dtype(dtype).name, tuple(sorted(changed.items())))
    if key not in _runs:
        _runs[key] = F.detect_ref(model, frame, fine=fine, dtype=dtype, **changed)
    return _runs[key]


def _key(r, shift=0):
    return (r["level"] + shift, r["component"], r["root_y"], r["root_x"], np.float32(r["score"]).tobytes(), r["parts"].tobytes())


def _min_side(recs):
    return min(int(min(r["parts"][0][2], r["parts"][0][3])) for r in recs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_equals_the_oracle(oracle, model, frame, dtype):
    want = oracle.detect(model.flatten(), frame, dtype)
    got = _run(model, frame, False, dtype)
    assert len(want) == 446
    assert [_key(r) for r in got] == [_key(r) for r in want]
    assert [_key(r) for r in got] == [_key(r) for r in P.detect_ref(model, frame, 0, 0, dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_levels_are_unchanged(oracle, model, frame, dtype):
    off, on = _run(model, frame, False, dtype), _run(model, frame, True, dtype)
    feats, _ = oracle.features_pyramid(model.flatten(), frame, dtype)
    nf = F.nfine(model.interval, len(feats))
    assert nf == 5
    assert [_key(r) for r in on if r["level"] >= nf] == [_key(r, nf) for r in off]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fine_levels_hold_what_no_other_setting_reaches(model, frame, dtype):
    off, on = _run(model, frame, False, dtype), _run(model, frame, True, dtype)
    nf = 5
    for l in range(nf):
        assert any(r["level"] == l for r in on), l
    assert _min_side([r for r in on if r["level"] < nf]) < _min_side(off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_half_size_object(oracle, dtype):
    """The patch of fineoctave_cases.planted (seed 3), pasted at half size at (y, x) = (18, 26).  Best score with the octave off:
    10.632 (level 0, rectangle (24, 16, 19, 19)); with it on: 15.277 at fine level 0, rectangle (28, 20, 9, 9) against the pasted
    interior (28, 20, 10, 10).  The threshold 13.0 lies between the two."""
    model, im, (bx, by, side) = cases.planted(oracle)
    assert F.detect_ref(model, im, fine=False, dtype=dtype) == []
    found = F.detect_ref(model, im, fine=True, dtype=dtype)
    assert len(found) >= 1
    best = max(found, key=lambda r: r["score"])
    _, scales = F.features_pyramid(model.flatten(), im, dtype)
    cell = float(scales[best["level"]])
    assert best["level"] < model.interval and cell == 2.0
    x, y, w, h = (int(v) for v in best["parts"][0])
    assert abs(x - bx) <= cell and abs(y - by) <= cell and abs(w - side) <= cell and abs(h - side) <= cell
    # the scores the docstring states, and that the threshold separates them
    loose = M.Model(**{**model.__dict__, "thresh": -1e9})
    off = max(r["score"] for r in F.detect_ref(loose, im, fine=False, dtype=dtype))
    assert abs(off - 10.632) < 0.01 and abs(best["score"] - 15.277) < 0.01 and off < cases.PLANT_THRESH < best["score"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("changed", [{"scale_div": 1}, {"image_shift": 1}, {"sbin": 4}], ids=["scale", "image", "sbin"])
def test_a_changed_rule_changes_the_records(model, frame, dtype, changed):
    right = [_key(r) for r in _run(model, frame, True, dtype)]
    wrong = [_key(r) for r in _run(model, frame, True, dtype, **changed)]
    assert wrong != right
    assert [k for k in wrong if k[0] >= 5] == [k for k in right if k[0] >= 5]     # only the fine levels follow the rule


@pytest.mark.parametrize("sbin", [4, 6, 8])
def test_plan_arithmetic(oracle, sbin):
    for rows, cols, interval in [(96, 128, 5), (103, 155, 3), (140, 268, 10), (200, 190, 2)]:
        lr, lc, sc = oracle.pyramid_plan(rows, cols, sbin, interval)
        ir, ic, fr, fc, scales, nf = F.plan(rows, cols, sbin, interval)
        n = len(lr)
        assert nf == min(interval, n) and len(ir) == len(fr) == len(scales) == n + nf
        assert np.array_equal(ir[:nf], lr[:nf]) and np.array_equal(ic[:nf], lc[:nf])
        assert np.array_equal(ir[nf:], lr) and np.array_equal(ic[nf:], lc) and scales[nf:].tobytes() == sc.tobytes()
        for i in range(nf):
            assert (fr[i], fc[i]) == oracle.hog_dims(int(lr[i]), int(lc[i]), sbin // 2)
            assert fr[i] == max(int(np.floor(np.float32(lr[i]) / np.float32(sbin // 2) + np.float32(0.5))) - 2, 0)
            assert np.float32(scales[i]) * np.float32(2) == sc[i]          # an exact halving
        for l in range(n):
            assert (fr[nf + l], fc[nf + l]) == oracle.hog_dims(int(lr[l]), int(lc[l]), sbin)


@pytest.mark.parametrize("sbin", [2, 3, 5])
def test_bin_sizes_without_a_fine_octave_are_refused(sbin):
    with pytest.raises(ValueError):
        F.fine_sbin(sbin)
    with pytest.raises(ValueError):
        F.plan(48, 64, sbin, 5)
    model = M.synthetic_model(seed=3, pa=[0, 1], nmix=1, sbin=sbin, interval=2, name="odd")
    with pytest.raises(ValueError):
        F.detect_ref(model, synthetic_frame(5, 48, 64), fine=True)


def test_too_many_levels_are_refused(oracle):
    lr, _, _ = oracle.pyramid_plan(300, 300, 4, 30)
    assert len(lr) == 118 and len(lr) + 30 > F.MAX_LEVELS >= len(lr)
    with pytest.raises(ValueError):
        F.plan(300, 300, 4, 30)


def test_position_plane_edge_sizes():
    """the frames of the GPU test's uint8 / int16 threshold: fine level 0's longest side is 256 and 258 cells, the base level's
    127 and 128"""
    for cols, fine_side, base_side in [(516, 256, 127), (520, 258, 128)]:
        _, _, fr, fc, _, nf = F.plan(40, cols, 4, 5)
        assert max(fr[0], fc[0]) == fine_side and max(fr[nf], fc[nf]) == base_side
        assert max(int(fr.max()), int(fc.max())) == fine_side
