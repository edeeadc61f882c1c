"""Warped positives on the CPU: the numpy yardstick of pbd_warp_positives* (partsbaseddetector_amd/warp.py) against a literal
restatement of the reference's Matlab code, its example format, and the C++ host mirror's members.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from partsbaseddetector_amd import examples as ex
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_part_model(k, sbin=4, seed=5):
    return M.synthetic_model(seed=seed, pa=[0], nmix=1, ksize=k, sbin=sbin, interval=5, name=f"one_part_k{k}_s{sbin}")


def frame(rows, cols, cn=3, seed=0, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols, cn)).astype(dtype)


# ---- warppos.m:21-26 and subarray.m, literally, in Matlab's 1-based coordinates ---------------------------------------------
def matlab_round(v):
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)   # halves away from zero (small exact arguments only)


def matlab_window_pixels(rows, cols, box, k, sbin):
    """the (i, j) 1-based source pixel of every window pixel, by subarray's loop with pad = 1; box is 0-based inclusive"""
    x1, y1, x2, y2 = (v + 1 for v in box)                # pos(i).x1 ... as Matlab holds them
    pixels = (k * sbin, k * sbin)
    widths, heights = x2 - x1 + 1, y2 - y1 + 1
    padx = sbin * widths / pixels[1]
    pady = sbin * heights / pixels[0]
    X1, X2 = matlab_round(x1 - padx), matlab_round(x2 + padx)
    Y1, Y2 = matlab_round(y1 - pady), matlab_round(y2 + pady)
    B = np.zeros((Y2 - Y1 + 1, X2 - X1 + 1, 2), np.int64)
    for i in range(Y1, Y2 + 1):
        for j in range(X1, X2 + 1):
            ii = min(max(i, 1), rows)
            jj = min(max(j, 1), cols)
            B[i - Y1, j - X1] = (ii, jj)
    return B


WINDOW_CASES = [
    # (rows, cols, box, k, sbin)
    (80, 96, (20, 20, 59, 49), 5, 4),      # inside
    (80, 96, (2, 30, 40, 60), 5, 4),       # crosses the left edge
    (80, 96, (60, 30, 94, 60), 5, 4),      # right
    (80, 96, (30, 1, 60, 40), 5, 4),       # top
    (80, 96, (30, 50, 60, 78), 5, 4),      # bottom
    (80, 96, (0, 0, 30, 30), 3, 8),        # top and left at once
    (80, 96, (70, 60, 95, 79), 3, 8),      # bottom and right at once
    (80, 96, (-60, -50, -20, -10), 5, 4),  # wholly outside, above and left
    (80, 96, (120, 100, 150, 140), 6, 4),  # wholly outside, below and right
    (80, 96, (10, 10, 10, 10), 5, 4),      # 1 x 1
    (80, 96, (0, 0, 0, 0), 1, 4),          # 1 x 1 at the corner, pad 1
    (80, 96, (0, 0, 2, 2), 6, 4),          # x - pad = 1 - 0.5 = 0.5: Matlab rounds to 1 (0-based 0)
    (80, 96, (-1, -1, 1, 1), 6, 4),        # 0 - 0.5 = -0.5 rounds to -1 (0-based -2): round(x1 - pad) 0-based would give 0 / -2 wrongly
    (80, 96, (-2, 3, 0, 5), 2, 8),         # -1 - 1.5 = -2.5 rounds to -3
    (80, 96, (5, 5, 9, 9), 10, 4),         # pad 0.5 on both sides of positive coordinates
]


@pytest.mark.parametrize("rows,cols,box,k,sbin", WINDOW_CASES)
def test_window_is_warppos_and_subarray(rows, cols, box, k, sbin):
    B = matlab_window_pixels(rows, cols, box, k, sbin)
    x0, y0, w, h = warp.window(box, k, sbin)
    assert (h, w) == B.shape[:2]
    ys = np.clip(np.arange(y0, y0 + h), 0, rows - 1) + 1
    xs = np.clip(np.arange(x0, x0 + w), 0, cols - 1) + 1
    assert np.array_equal(B[:, :, 0], np.repeat(ys[:, None], w, 1))
    assert np.array_equal(B[:, :, 1], np.repeat(xs[None, :], h, 0))
    # and the gather itself
    im = frame(rows, cols, 3, seed=1)
    assert np.array_equal(warp.crop(im, box, k, sbin), im[B[:, :, 0] - 1, B[:, :, 1] - 1])


def test_half_rounding_differs_from_a_zero_based_shortcut():
    """round() of the 0-based coordinate differs from Matlab's 1-based one exactly where x - pad lands on a half at or below
    zero: the yardstick follows Matlab"""
    x0, _, _, _ = warp.window((-1, -1, 1, 1), 6, 4)       # pad 0.5: 1-based 0 - 0.5 = -0.5 -> -1 -> 0-based -2
    assert x0 == -2
    assert warp.matlab_round(-1 - 0.5) == -2              # the 0-based shortcut gives the same here ...
    x0, _, _, _ = warp.window((0, 0, 2, 2), 6, 4)         # ... but not here: 1-based 1 - 0.5 = 0.5 -> 1 -> 0-based 0
    assert x0 == 0 and warp.matlab_round(0 - 0.5) == -1
    for v, r in [(0.5, 1), (-0.5, -1), (1.5, 2), (-2.5, -3), (0.49999999999999994, 0), (2.4, 2), (-2.6, -3)]:
        assert warp.matlab_round(v) == r


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 3), (np.uint8, 1), (np.uint16, 3), (np.float32, 3), (np.float64, 1)])
def test_identity_patch_is_the_crop(dtype, cn):
    """a window of exactly P x P pixels inside the frame: the resize is the identity, byte for byte, and the example's filter
    block is the HOG of the plain crop"""
    k, sbin = 5, 4
    P = (k + 2) * sbin                                     # 28; width 20 pads by 4 per side
    box = (30, 25, 30 + k * sbin - 1, 25 + k * sbin - 1)
    x0, y0, w, h = warp.window(box, k, sbin)
    assert (w, h) == (P, P) and x0 >= 0 and y0 >= 0
    im = frame(80, 96, cn, seed=2, dtype=dtype)
    if dtype in (np.float32, np.float64):
        im = im / dtype(3)
    cropped = im[y0:y0 + P, x0:x0 + P]
    assert warp.patch(im, box, k, sbin).tobytes() == np.ascontiguousarray(cropped).tobytes()
    flat = one_part_model(k, sbin).flatten()
    for T in (np.float32, np.float64):
        hdr, vals, kept = warp.warp_examples(flat, [im], [(0,) + box], 0, 0, True, T)
        assert kept.tolist() == [1]
        feat = oracle.hog_features(np.ascontiguousarray(cropped), sbin, dtype=T)
        assert vals[0, 0] == 1 and vals[0, 1:1 + feat.size].tobytes() == feat.tobytes()


def test_window_wholly_outside_gives_zero_features():
    k, sbin = 3, 4
    flat = one_part_model(k, sbin).flatten()
    im = frame(80, 96, 3, seed=3)
    box = (-80, -70, -30, -20)
    p = warp.patch(im, box, k, sbin)
    assert (p == im[0, 0]).all()                           # the corner pixel, replicated
    hdr, vals, kept = warp.warp_examples(flat, [im], [(0,) + box], 0, 0, True)
    n = k * k * flat.flen
    assert kept[0] == 1 and vals[0, 0] == 1 and not vals[0, 1:1 + n].any()


def test_header_layout_bias_forms_and_skip_rule():
    k, sbin = 3, 4
    m = M.synthetic_model(seed=7, pa=[0, 1], nmix=2, ksize=k, sbin=sbin, interval=5)
    flat = m.flatten()
    hw, vw = ex.strides(flat)
    dbase, fbase, _ = ex.vector_offsets(flat)
    im = frame(80, 96, 3, seed=4)
    side = k * sbin                                        # minsize = side^2 = 144
    boxes = [(0, 10, 10, 10 + side - 1, 10 + side - 1),    # area == minsize: kept
             (0, 10, 10, 10 + side - 1, 10 + side - 2),    # area == minsize - side: skipped
             (0, 5, 5, 5 + 142, 5),                        # 143 x 1 = minsize - 1: skipped
             (0, 5, 5, 5 + 143, 5)]                        # 144 x 1 = minsize: kept
    f, b = 2, 3
    hdr, vals, kept = warp.warp_examples(flat, [im], boxes, f, b, True)
    assert hdr.shape == (4, hw) and vals.shape == (4, vw) and kept.tolist() == [1, 0, 0, 1]
    n = k * k * flat.flen
    for i in (0, 3):
        assert hdr[i, :8].tolist() == [i, 0, 2, 1 + n, b, 1, fbase + int(flat.filter_offset[f]), n] and not hdr[i, 8:].any()
        assert vals[i, 0] == 1 and not vals[i, 1 + n:].any()
    for i in (1, 2):                                       # the invalid marker pbd_qp_add_device skips
        assert hdr[i].tolist() == [i, 0, -1] + [0] * (hw - 3) and not vals[i].any()
    # without the rule every box is kept
    assert warp.warp_examples(flat, [im], boxes, f, b, False)[2].tolist() == [1, 1, 1, 1]
    # bias -1: the filter block alone
    h2, v2, _ = warp.warp_examples(flat, [im], boxes[:1], f, -1, True)
    assert h2[0, :6].tolist() == [0, 0, 1, n, fbase + int(flat.filter_offset[f]), n] and not h2[0, 6:].any()
    assert v2[0, :n].tobytes() == vals[0, 1:1 + n].tobytes() and not v2[0, n:].any()
    # w . x of the example = bias + filter . features
    w = ex.model_vector(flat)
    o = fbase + int(flat.filter_offset[f])
    want = float(w[b]) + float(np.dot(w[o:o + n].astype(np.float64), vals[0, 1:1 + n].astype(np.float64)))
    assert ex.dot(hdr[0], vals[0], w)[0] == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_warp_members_compile(tmp_path, std):
    """include/pbd_host.hpp warpPositives / warpPositivesDevice compile for T = float and double"""
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
size_t use(pbdhost::PartsBasedDetector<T> &d)
{
    std::vector<pbdhost::Image> ims(1);
    std::vector<int32_t> boxes(5, 0), hdr;
    std::vector<T> values;
    std::vector<bool> kept;
    int hdr_words = 0, nvalues = 0;
    d.warpPositives(ims, boxes, 0, 0, true, hdr, values, kept, hdr_words, nvalues);
    std::vector<pbd_frame> frames(1);
    d.warpPositivesDevice(frames, 3, 0, boxes, 0, -1, false, 7, (int32_t *)0, 1, (int32_t *)0, (T *)0);
    return hdr.size() + values.size() + kept.size() + (size_t)hdr_words + (size_t)nvalues;
}
template size_t use<float>(pbdhost::PartsBasedDetector<float> &);
template size_t use<double>(pbdhost::PartsBasedDetector<double> &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
