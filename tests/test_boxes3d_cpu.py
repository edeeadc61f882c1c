"""Candidate.boundingBox3D, the numpy mirror of include/Candidate.hpp:140-216 that the device stage (pbd_boxes3d) is held to,
against formulations that do not share its code: closed-form scenes, a plain-Python restatement with scalar float32 steps,
and brute-force order statistics.  No GPU: only the C++ readPNM test compiles a small program."""
import math
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import synth
from partsbaseddetector_amd.detector import Candidate, _resize_linear_400

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def cand(parts):
    parts = np.asarray(parts, np.int32).reshape(-1, 4)
    return Candidate(parts=parts, confidence=np.zeros(len(parts), np.float32), component=0)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def bits(t):
    return np.array(t, np.float64).view(np.uint64)


# ---- a plain restatement, scalar by scalar -------------------------------------------------------------------------------------
def slow_box3d(parts, rows, cols, depth):
    def inter(a, b):
        x1, y1 = max(a[0], b[0]), max(a[1], b[1])
        w, h = min(a[0] + a[2], b[0] + b[2]) - x1, min(a[1] + a[3], b[1] + b[3]) - y1
        return [x1, y1, w, h] if w > 0 and h > 0 else [0, 0, 0, 0]
    n = len(parts)
    cx = [round((2 * p[0] + p[2]) / 2) for p in parts]
    cy = [round((2 * p[1] + p[3]) / 2) for p in parts]
    sx = math.sqrt(max(sum(v * v for v in cx) * (1.0 / n) - (sum(cx) * (1.0 / n)) ** 2, 0.0))   # exact integer sums
    sy = math.sqrt(max(sum(v * v for v in cy) * (1.0 / n) - (sum(cy) * (1.0 / n)) ** 2, 0.0))
    mean_x, mean_y = sum(cx) * (1.0 / n), sum(cy) * (1.0 / n)
    norm = [int(mean_x - 1.5 * sx), int(mean_y - 1.5 * sy), int(3 * sx), int(3 * sy)]
    boxes = [inter(list(p), [0, 0, cols, rows]) for p in parts] + [inter(norm, [0, 0, cols, rows])]
    drows, dcols = depth.shape
    kx, ky = dcols / cols, drows / rows
    pts = []
    for b in boxes:
        r = [int(b[0] * kx), int(b[1] * ky), int(b[2] * kx), int(b[3] * ky)]
        if r[2] <= 0 or r[3] <= 0:
            continue
        for yy in range(r[1], r[1] + r[3]):
            for xx in range(r[0], r[0] + r[2]):
                v = F32(depth[yy, xx])
                if v != 0 and not np.isnan(v):
                    pts.append(v)
        if not pts:
            return (math.nan, math.nan, math.nan, 0.0, 0.0, 0.0)
    if not pts:
        return (math.nan, math.nan, math.nan, 0.0, 0.0, 0.0)
    S = sorted(pts)
    M = len(S)
    p = []
    for dy in range(400):
        if M == 400:
            p.append(S[dy])
            continue
        fy = F32((dy + 0.5) * (1.0 / (400.0 / M)) - 0.5)
        s0 = math.floor(fy)
        fy = F32(fy - F32(s0))
        a, b = S[min(max(s0, 0), M - 1)], S[min(max(s0 + 1, 0), M - 1)]
        p.append(F32(F32(a * F32(F32(1) - fy)) + F32(b * fy)))
    g = [F32(math.exp(-0.03125 * (i - 17) ** 2)) for i in range(35)]
    tot = 0.0
    for v in g:
        tot += float(v)
    g = [F32(float(v) * (1.0 / tot)) for v in g]
    dog = [F32(g[i + 1 if i < 34 else 33] - g[abs(i - 1)]) for i in range(35)]   # [-1 0 1], reflect-101 ends
    d = []
    for m in range(400):
        s = F32(0)
        for t in range(35):
            if dog[t] == 0:
                continue
            j = abs(m + t - 17)
            if j > 399:
                j = 798 - j
            s = F32(s + F32(dog[t] * p[j]))
        d.append(s)
    hi = lo = 200
    for m in range(200, 400):
        if float(abs(d[m])) > 0.035:
            break
        hi = m
    for m in range(200, -1, -1):
        if float(abs(d[m])) > 0.035:
            break
        lo = m
    x, y, w, h = cand(parts).boundingBox()
    return (float(x), float(y), float(p[lo]), float(h), float(w), float(p[hi]) - float(p[lo]))


# ---- closed-form scenes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("area", [(20, 20), (21, 19), (40, 30)])
def test_constant_depth(area):
    c_val = F32(1.7)
    depth = np.full((480, 640), c_val, np.float32)
    w, h = area
    c = cand([[100, 120, w, h]])                         # one part: boundingBoxNorm is empty, M = w * h
    x, y, z, hh, ww, dd = c.boundingBox3D((480, 640), depth)
    assert (x, y, ww, hh) == (100.0, 120.0, float(w), float(h))
    if w * h == 400:
        assert z == float(c_val) and dd == 0.0
    else:
        assert ulps(z, c_val) <= 2 and abs(dd) <= 2 * float(np.spacing(c_val))
    parts = [[-30, 10, 50, 60], [600, 400, 100, 100], [200, 200, 10, 10]]
    x, y, z, hh, ww, dd = cand(parts).boundingBox3D((480, 640), depth)
    assert (x, y, ww, hh) == (-30.0, 10.0, 730.0, 490.0)   # the unclipped hull
    assert ulps(z, c_val) <= 2


def test_two_levels_stop_before_the_step():
    depth = np.full((100, 100), F32(2.0), np.float32)
    depth[70:, :] = F32(4.0)                             # 70 % of the one box's samples are 2.0, 30 % 4.0
    z = cand([[0, 0, 100, 100]]).boundingBox3D((100, 100), depth)
    assert ulps(z[2], 2.0) <= 2 and ulps(z[2] + z[5], 2.0) <= 2


@pytest.mark.parametrize("m", [1, 2, 399, 400, 401, 12345])
def test_resampled_ranks_brute_force(m):
    rng = np.random.default_rng(m)
    S = np.sort(rng.integers(-50, 50, m).astype(np.float32) / F32(8))
    p = _resize_linear_400(S)
    assert p.dtype == np.float32 and p.shape == (400,)
    for dy in range(400):
        if m == 400:
            assert p[dy] == S[dy]
            continue
        fy = F32((dy + 0.5) * (1.0 / (400.0 / m)) - 0.5)
        sy = int(math.floor(fy))
        fy = F32(fy - F32(sy))
        r0, r1 = min(max(sy, 0), m - 1), min(max(sy + 1, 0), m - 1)
        assert p[dy].view(np.int32) == F32(F32(S[r0] * F32(F32(1) - fy)) + F32(S[r1] * fy)).view(np.int32), dy


# ---- NaN boxes ---------------------------------------------------------------------------------------------------------------------
def test_nan_boxes():
    depth = np.full((480, 640), F32(3.0), np.float32)
    depth[0:50, 0:50] = 0
    nan_box = bits((math.nan, math.nan, math.nan, 0.0, 0.0, 0.0))
    assert (bits(cand([[0, 0, 50, 50], [100, 100, 20, 20]]).boundingBox3D((480, 640), depth)) == nan_box).all()
    # leading boxes outside the frame are skipped, the first non-empty one has samples
    assert not np.isnan(cand([[-60, 0, 50, 50], [100, 100, 20, 20]]).boundingBox3D((480, 640), depth)[2])
    # every box empty: a 2 x 3 depth image under a VGA frame (the reference asserts in cv::resize)
    assert (bits(cand([[10, 10, 100, 100]]).boundingBox3D((480, 640), np.ones((2, 3), np.float32))) == nan_box).all()
    # a box that is empty only after scaling (width 1 at half resolution), then a hole-only box: NaN box
    half = np.full((240, 320), F32(3.0), np.float32)
    half[100:120, 100:120] = 0
    assert (bits(cand([[50, 50, 1, 30], [200, 200, 40, 40]]).boundingBox3D((480, 640), half)) == nan_box).all()
    assert not np.isnan(cand([[50, 50, 1, 30], [300, 300, 40, 40]]).boundingBox3D((480, 640), half)[2])


# ---- against the scalar restatement ---------------------------------------------------------------------------------------------
PARTS = [[5 + 24 * k, 7 + 17 * k, 9 + k, 8 + (k % 5)] for k in range(26)]


@pytest.mark.parametrize("dshape", [(480, 640), (240, 320), (370, 500)])
def test_mirror_equals_scalar_restatement(dshape):
    depth = synth.synthetic_depth(4, dshape[0], dshape[1], np.float32, inf=True)
    for parts in (PARTS, PARTS[:5], PARTS[10:12]):
        assert (bits(cand(parts).boundingBox3D((480, 640), depth)) == bits(slow_box3d(parts, 480, 640, depth))).all()


def test_16u_equals_32f_and_64f_rounding():
    d16 = synth.synthetic_depth(8, 370, 500, np.uint16)
    for parts in (PARTS, PARTS[3:9]):
        c = cand(parts)
        a = c.boundingBox3D((480, 640), d16)
        assert (bits(a) == bits(c.boundingBox3D((480, 640), d16.astype(np.float32)))).all()
        assert (bits(a) == bits(slow_box3d(parts, 480, 640, d16))).all()
    d64 = np.full((50, 50), 2.0)
    d64[:, :25] = 1e-50                                   # rounds to 0.0f: excluded
    c = cand([[0, 0, 50, 50]])
    ref = np.full((50, 25), F32(2.0), np.float32)
    got = c.boundingBox3D((50, 50), d64)
    assert got[2] == 2.0 and got[5] == 0.0 and np.isfinite(got).all()
    assert (bits(got[2:3]) == bits(cand([[0, 0, 25, 50]]).boundingBox3D((50, 25), ref)[2:3])).all()


def test_bounding_box_norm_ties_and_truncation():
    # centroids (2x + w) / 2 with odd sums: x = 0, w = 1 -> 0.5 -> 0; x = 1, w = 1 -> 1.5 -> 2; x = 2, w = 1 -> 2.5 -> 2
    c = cand([[0, 0, 1, 1], [1, 1, 1, 1], [2, 2, 1, 1]])
    cx = [0, 2, 2]
    mean = sum(cx) / 3
    sd = math.sqrt(max(sum(v * v for v in cx) * (1.0 / 3) - (sum(cx) * (1.0 / 3)) ** 2, 0.0))
    assert c.boundingBoxNorm() == (int(mean - 1.5 * sd), int(mean - 1.5 * sd), int(3 * sd), int(3 * sd))
    # negative means: truncation toward zero, not floor
    c = cand([[-41, -31, 1, 1], [-37, -29, 2, 2]])     # centroids x: -40.5 -> -40, -36 ; y: -30.5 -> -30, -28
    mx, my = (-40 - 36) / 2, (-30 - 28) / 2
    sx, sy = 2.0, 1.0
    assert c.boundingBoxNorm() == (int(mx - 1.5 * sx), int(my - 1.5 * sy), 6, 3)
    assert int(mx - 1.5 * sx) == -41 and int(my - 1.5 * sy) == -30   # -41.0 and -30.5 truncated toward zero


# ---- readPNM (C++ host header) ----------------------------------------------------------------------------------------------------
def test_read_pnm_8_and_16_bit(tmp_path):
    src = tmp_path / "pnm.cpp"
    src.write_text(r'''
#include "pbd_host.hpp"
#include <cstdio>
int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<uint8_t> pix; pbdhost::Image im;
        if (!pbdhost::readPNM(argv[i], pix, im)) { std::printf("fail\n"); continue; }
        unsigned long long sum = 0;
        for (int y = 0; y < im.rows; ++y)
            for (int x = 0; x < im.cols * im.channels; ++x)
                { const uint8_t *row = static_cast<const uint8_t *>(im.data) + y * im.step; sum += im.depth == 2 ? reinterpret_cast<const uint16_t *>(row)[x] : row[x]; }
        std::printf("%d %d %d %d %llu\n", im.rows, im.cols, im.channels, im.depth, sum);
    }
}
''')
    exe = tmp_path / "pnm"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rng = np.random.default_rng(1)
    a8 = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    a16 = rng.integers(0, 65536, (5, 7), dtype=np.uint16)
    p8, p16, pbig = tmp_path / "a.pgm", tmp_path / "b.pgm", tmp_path / "c.pgm"
    p8.write_bytes(b"P5\n7 5\n255\n" + a8.tobytes())
    p16.write_bytes(b"P5\n7 5\n65535\n" + a16.astype(">u2").tobytes())
    pbig.write_bytes(b"P5\n7 5\n1000\n" + a16.astype(">u2").tobytes())      # other maxvals stay unsupported
    out = subprocess.check_output([str(exe), str(p8), str(p16), str(pbig)]).decode().split("\n")
    assert out[0] == f"5 7 1 0 {int(a8.astype(np.int64).sum())}"
    assert out[1] == f"5 7 1 2 {int(a16.astype(np.int64).sum())}"
    assert out[2] == "fail"
