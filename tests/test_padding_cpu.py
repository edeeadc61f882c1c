"""CPU tests of the padded pyramid's rule (partsbaseddetector_amd/padding.py) against the oracle: the
unpadded case is oracle.detect, the interior of the padded responses is the unpadded responses, the record counts are pinned,
padded runs place parts left of anything the unpadded detector can produce, and a changed rule changes the records."""
import numpy as np
import pytest

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import padding as P
from partsbaseddetector_amd import synthetic_frame

PADS = [(2, 2), (1, 3), (7, 5)]
COUNTS = {(0, 0): 446, (2, 2): 986, (1, 3): 996, (7, 5): 2672}
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def model():
    return M.synthetic_tiny_model(thresh=-1.0)


@pytest.fixture(scope="module")
def frame():
    return synthetic_frame(5, 48, 64)


_runs = {}


def _run(model, frame, pad, dtype):
    key = (pad, np.dtype(dtype).name)
    if key not in _runs:
        _runs[key] = P.detect_ref(model, frame, pad[0], pad[1], dtype)
    return _runs[key]


def _same(a, b):
    return len(a) == len(b) and all(
        (g["level"], g["component"], g["root_y"], g["root_x"]) == (w["level"], w["component"], w["root_y"], w["root_x"])
        and np.float32(g["score"]) == np.float32(w["score"]) and np.array_equal(g["parts"], w["parts"]) for g, w in zip(a, b))


def _left_of_frame(oracle, model, frame, recs, dtype):
    """part boxes whose x1 lies left of -scale - 1: the unpadded detector's leftmost rectangle starts at round(-scale)"""
    _, scales = oracle.features_pyramid(model.flatten(), frame, dtype)
    return sum(int(np.sum(r["parts"][:, 0] < -float(scales[r["level"]]) - 1)) for r in recs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpadded_is_the_oracle(oracle, model, frame, dtype):
    want = oracle.detect(model.flatten(), frame, dtype)
    got = _run(model, frame, (0, 0), dtype)
    assert len(want) == COUNTS[(0, 0)]
    assert _same(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", PADS)
def test_interior_responses_are_the_unpadded_ones(oracle, model, frame, pad, dtype):
    flat = model.flatten()
    feats, _ = oracle.features_pyramid(flat, frame, dtype)
    assert feats[-1].shape == (3, 5 * flat.flen)        # (7, 5) is larger than the last level
    for f in feats:
        H, W = f.shape[0], f.shape[1] // flat.flen
        padded = oracle.responses(flat, P.pad_features(f, pad[0], pad[1], flat.flen))
        inner = np.ascontiguousarray(padded[:, pad[1]:pad[1] + H, pad[0]:pad[0] + W])
        assert inner.tobytes() == oracle.responses(flat, f).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", PADS)
def test_record_counts_and_parts_outside_the_frame(oracle, model, frame, pad, dtype):
    recs = _run(model, frame, pad, dtype)
    assert len(recs) == COUNTS[pad]
    assert _left_of_frame(oracle, model, frame, recs, dtype) > 0
    assert _left_of_frame(oracle, model, frame, _run(model, frame, (0, 0), dtype), dtype) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", PADS)
def test_rectangles_without_the_pad_offset_differ(model, frame, pad, dtype):
    right = _run(model, frame, pad, dtype)
    wrong = P.detect_ref(model, frame, pad[0], pad[1], dtype, rect_pad=(0, 0))
    assert len(wrong) == len(right) and not _same(wrong, right)


@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_walk_keeps_the_roots(model, frame, dtype):
    ref = _run(model, frame, (2, 2), dtype)
    arg = P.detect_ref(model, frame, 2, 2, dtype, walk="argmax")
    assert [(r["level"], r["component"], r["root_y"], r["root_x"], r["score"]) for r in arg] == \
           [(r["level"], r["component"], r["root_y"], r["root_x"], r["score"]) for r in ref]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pad_cells(dtype):
    rng = np.random.default_rng(3)
    f = -np.abs(rng.standard_normal((3, 5 * 32))).astype(dtype)
    g = P.pad_features(f, 2, 1).reshape(5, 9, 32)
    assert np.array_equal(g[1:4, 2:7].reshape(3, -1), f)
    mask = np.ones((5, 9), bool)
    mask[1:4, 2:7] = False
    pad = g[mask]
    assert np.all(pad[:, :31] == 0) and not np.any(np.signbit(pad[:, :31])) and np.all(pad[:, 31] == 1)
    for shape in [(0, 5 * 32), (3, 0), (0, 0)]:
        assert P.pad_features(np.zeros(shape, dtype), 2, 1).size == 0
    assert P.pad_features(f, 0, 0).tobytes() == f.tobytes()
    for bad in [(-1, 0), (0, 32), (32, 32)]:
        with pytest.raises(ValueError):
            P.pad_features(f, *bad)


def test_ptr8_edge_sizes(oracle):
    """the frames of the GPU test's uint8 / int16 pointer threshold: level 0 is 8 x 250 (250 x 8) cells, so padx = 3 gives a
    longest padded side of exactly 256 and padx = 4 one of 258"""
    model = M.synthetic_tiny_model()
    for rows, cols in [(40, 1008), (1008, 40)]:
        lr, lc, _ = oracle.pyramid_plan(rows, cols, model.sbin, model.interval)
        H, W = oracle.hog_dims(int(lr[0]), int(lc[0]), model.sbin)
        assert (H, W) == ((8, 250) if rows == 40 else (250, 8))
        assert max(H, W) + 2 * 3 == 256 and max(H, W) + 2 * 4 == 258
