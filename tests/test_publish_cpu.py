"""The numpy yardsticks of the candidate mask and the part-centre poses (partsbaseddetector_amd/publish.py) pinned against literal
restatements: Candidate::mask as a loop of setTo(n+1, mask == 0) with saturation, `rgb & (mask != 0)` per byte, and PCL's
per-point computeMeanAndCovarianceMatrix loop; the eigen-frame against numpy.linalg.eigh.  Also the new symbols and the refusals
that need no GPU.  No GPU is used here."""
import ctypes as C
import math

import numpy as np
import pytest

from partsbaseddetector_amd import publish
from partsbaseddetector_amd.pointcloud import jacobi3

F = np.float32
MAX_PARTS = 4
STRIDE = 8 + 4 * MAX_PARTS


def literal_mask(rows, cols, boxes):
    """Candidate::mask: for n in order, box = boundingBox & bounds, mask(box).setTo(saturate_cast<uchar>(n+1), mask(box) == 0)"""
    mask = np.zeros((rows, cols), np.uint8)
    for n, (x, y, w, h) in enumerate(boxes):
        x1, y1 = max(x, 0), max(y, 0)
        x2, y2 = min(x + w, cols), min(y + h, rows)
        if x2 - x1 <= 0 or y2 - y1 <= 0:
            continue
        v = min(n + 1, 255)
        for r in range(y1, y2):
            for c in range(x1, x2):
                if mask[r, c] == 0:
                    mask[r, c] = v
    return mask


def literal_hull(parts):
    """cv::Rect operator|= over the parts, starting from parts[0]"""
    x, y, w, h = parts[0]
    for bx, by, bw, bh in parts:
        if w <= 0 or h <= 0:
            x, y, w, h = bx, by, bw, bh
        elif bw > 0 and bh > 0:
            x1, y1 = min(x, bx), min(y, by)
            w, h = max(x + w, bx + bw) - x1, max(y + h, by + bh) - y1
            x, y = x1, y1
    return x, y, w, h


def random_records(rng, n, rows, cols, frame=0, empty_every=0):
    rec = np.zeros((n, STRIDE), np.int32)
    for i in range(n):
        np_ = int(rng.integers(1, MAX_PARTS + 1))
        rec[i, 0] = frame
        rec[i, 6] = np_
        for j in range(np_):
            w, h = int(rng.integers(-3, cols // 3)), int(rng.integers(-3, rows // 3))
            if empty_every and i % empty_every == 0:
                w = -abs(w)                  # empty parts: the hull may be empty too
            rec[i, 8 + 4 * j:12 + 4 * j] = (int(rng.integers(-cols // 4, cols)), int(rng.integers(-rows // 4, rows)), w, h)
    return rec


def test_record_boxes_are_the_hull():
    rng = np.random.default_rng(1)
    rec = random_records(rng, 200, 60, 80, empty_every=7)
    got = publish.record_boxes(rec)
    for i, r in enumerate(rec):
        parts = [tuple(int(v) for v in r[8 + 4 * j:12 + 4 * j]) for j in range(r[6])]
        assert tuple(got[i]) == literal_hull(parts)


@pytest.mark.parametrize("n", [0, 1, 30, 300, 700])
def test_mask_equals_the_literal_loop(n):
    rng = np.random.default_rng(n)
    rows, cols = 47, 61
    rec = random_records(rng, n, rows, cols, empty_every=5)
    boxes = publish.record_boxes(rec)
    want = literal_mask(rows, cols, [tuple(int(v) for v in b) for b in boxes])
    got = publish.candidate_mask((rows, cols), boxes)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_records_from_254_on_paint_255():
    boxes = [(i % 40, i // 40, 1, 1) for i in range(600)] + [(0, 0, 40, 20)]
    got = publish.candidate_mask((20, 40), boxes)
    assert np.array_equal(got, literal_mask(20, 40, boxes))
    assert got[0, 0] == 1 and got[6, 13] == 254 and got[6, 14] == 255 and got[19, 39] == 255


def test_boxes_partly_and_fully_outside_and_empty():
    rows, cols = 20, 30
    boxes = [(-5, -5, 10, 10), (25, 15, 10, 10), (40, 0, 5, 5), (0, 30, 5, 5), (3, 3, 0, 5), (3, 3, 5, -1), (-10, 2, 5, 5),
             (0, 0, 30, 20)]
    want = literal_mask(rows, cols, boxes)
    assert np.array_equal(publish.candidate_mask((rows, cols), boxes), want)
    assert want[0, 0] == 1 and want[19, 29] == 2 and want[10, 10] == 8


def test_several_frames_of_different_sizes():
    rng = np.random.default_rng(7)
    shapes = [(31, 45), (17, 80), (64, 20)]
    recs = [random_records(rng, k, s[0], s[1], frame=f + 5) for f, (s, k) in enumerate(zip(shapes, (40, 0, 300)))]
    rec = np.concatenate(recs)
    got = publish.frame_masks(shapes, rec, frame_offset=5)
    for f, s in enumerate(shapes):
        boxes = [tuple(int(v) for v in b) for b in publish.record_boxes(recs[f])]
        assert np.array_equal(got[f], literal_mask(s[0], s[1], boxes))


def test_candidate_mask_static_method_uses_bounding_box():
    from partsbaseddetector_amd.detector import Candidate
    c0 = Candidate(parts=np.array([[2, 2, 4, 4], [5, 5, 3, 3]], np.int32), confidence=np.zeros(2, F), component=0)
    c1 = Candidate(parts=np.array([[0, 0, 10, 3]], np.int32), confidence=np.zeros(1, F), component=0)
    got = Candidate.mask((9, 12), [c0, c1])
    assert np.array_equal(got, literal_mask(9, 12, [c0.boundingBox(), c1.boundingBox()]))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_masked_image_is_rgb_and_mask(cn):
    rng = np.random.default_rng(cn)
    rows, cols = 13, 17
    lab = rng.integers(0, 3, (rows, cols)).astype(np.uint8)
    im = rng.integers(0, 256, (rows, cols, cn)).astype(np.uint8)
    want = im.copy()
    for r in range(rows):
        for c in range(cols):
            for k in range(cn):
                want[r, c, k] = im[r, c, k] & (0xFF if lab[r, c] != 0 else 0)
    assert np.array_equal(publish.masked_image(im, lab), want)
    if cn == 1:
        assert np.array_equal(publish.masked_image(im[:, :, 0], lab), want[:, :, 0])


# ---- poses ---------------------------------------------------------------------------------------------------------------------
def literal_moments(pts, dense):
    """pcl::computeMeanAndCovarianceMatrix, one fp32 operation at a time, then the node's covMat /= point_count"""
    acc = [F(0)] * 9
    count = 0
    for x, y, z in pts:
        x, y, z = F(x), F(y), F(z)
        if not dense and not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            continue
        with np.errstate(all="ignore"):
            for k, v in enumerate((F(x * x), F(x * y), F(x * z), F(y * y), F(y * z), F(z * z), x, y, z)):
                acc[k] = F(acc[k] + v)
        count += 1
    if count == 0:
        return 0, None, None
    fc = F(count)
    with np.errstate(all="ignore"):
        m = [F(a / fc) for a in acc]
        c = [F(m[0] - F(m[6] * m[6])), F(m[1] - F(m[6] * m[7])), F(m[2] - F(m[6] * m[8])), F(m[3] - F(m[7] * m[7])),
             F(m[4] - F(m[7] * m[8])), F(m[5] - F(m[8] * m[8]))]
        c = [F(v / fc) for v in c]
    return count, m[6:9], c


def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def random_centres(rng, n, scale=1.0):
    cen = (rng.standard_normal((n, MAX_PARTS, 3)) * np.array([0.3, 0.2, 0.05]) * scale + np.array([0.1, -0.2, 2.0])).astype(F)
    nc = rng.integers(3, MAX_PARTS + 1, n).astype(np.int32)
    return cen, nc, np.ones(n, np.int32)


def test_moments_equal_the_literal_pcl_loop():
    rng = np.random.default_rng(3)
    cen, nc, dn = random_centres(rng, 40)
    cen[5, 1] = (np.nan, 0, 1)
    cen[6, 0] = (np.inf, 0, 1)
    cen[7, 2] = (0, -np.inf, 1)
    dn[5:8] = 0
    dn[8] = 1
    cen[8, 0] = (np.inf, 1, 1)
    cnt, pos, quat, ev = publish.part_poses(cen, nc, dn)
    for i in range(len(cen)):
        count, mean, c = literal_moments(cen[i, :nc[i]], bool(dn[i]))
        assert cnt[i] == count
        assert bits_equal(pos[i], mean)
    assert np.isnan(quat[8]).all() and np.isnan(ev[8]).all()          # dense with an Inf point: the covariance is not finite
    assert np.isfinite(quat[5:8]).all()                                # not dense: the non-finite points are skipped


def test_count_zero_one_and_two():
    cen = np.zeros((4, MAX_PARTS, 3), F)
    cen[1, 0] = (1, 2, 3)
    cen[2, :2] = ((1, 2, 3), (2, 2, 3))
    cen[3, :] = np.nan
    nc = np.array([0, 1, 2, 4], np.int32)
    dn = np.array([1, 1, 1, 0], np.int32)
    cnt, pos, quat, ev = publish.part_poses(cen, nc, dn)
    assert list(cnt) == [0, 1, 2, 0]
    for i in (0, 3):
        assert np.isnan(pos[i]).all() and np.isnan(quat[i]).all() and np.isnan(ev[i]).all()
    assert bits_equal(pos[1], [1, 2, 3])
    assert np.array_equal(ev[1], [0, 0, 0]) and np.array_equal(quat[1], [0, 0, 0, 1])   # a zero covariance: the identity frame
    assert bits_equal(pos[2], [1.5, 2, 3])
    assert ev[2][0] == 0 and ev[2][1] == 0 and ev[2][2] == F(0.25 / 2)   # spread 0.25 along x, divided by the count again


def rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_frame_against_eigh_and_quaternion_is_the_frame():
    rng = np.random.default_rng(11)
    cen, nc, dn = random_centres(rng, 200)
    cnt, pos, quat, ev = publish.part_poses(cen, nc, dn)
    checked = 0
    for i in range(len(cen)):
        _, _, c = literal_moments(cen[i, :nc[i]], True)
        Cm = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float64)
        w, v = np.linalg.eigh(Cm)
        lam, M = publish.pose_frame(Cm.tolist())
        M = np.array(M)
        assert bits_equal(ev[i], np.array(lam).astype(F))
        gaps = np.diff(w)
        if gaps.min() < 1e-6 * max(abs(w).max(), 1e-30):
            continue                                                   # ill-conditioned: eigenvectors not unique
        checked += 1
        assert np.allclose(lam, w, rtol=1e-9, atol=1e-9 * abs(w).max())
        for col in (0, 1):
            e = v[:, col]
            big = int(np.argmax(np.abs(e)))
            e = e if e[big] >= 0 else -e
            assert np.allclose(M[:, col], e, atol=1e-6)
        assert np.allclose(M[:, 2], np.cross(M[:, 0], M[:, 1]))
        R = rot(quat[i])
        assert np.allclose(R, M, atol=1e-6)
        assert abs(np.linalg.det(R) - 1) < 1e-6
    assert checked > 100


def test_jacobi_is_the_plane_fits():
    A = [[2.0, 0.5, 0.1], [0.5, 1.0, 0.2], [0.1, 0.2, 0.5]]
    B = [r[:] for r in A]
    V = jacobi3(B)
    lam, M = publish.pose_frame(A)
    assert sorted(B[k][k] for k in range(3)) == lam
    assert abs(np.linalg.det(np.array(M)) - 1) < 1e-12
    assert all(math.isfinite(v) for r in V for v in r)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from partsbaseddetector_amd import build, _lib
    build.build_hip()
    return _lib.load()


def test_symbols_and_null_handle_refusal(lib):
    from partsbaseddetector_amd import _lib
    for name in ("pbd_candidate_mask", "pbd_candidate_mask_device", "pbd_part_poses", "pbd_part_poses_device"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    for name in ("k_mk_hull", "k_mk_tile", "k_part_poses"):
        assert name in _lib.KERNELS
    rows = np.array([4], np.int32)
    lab = np.zeros(16, np.uint8)
    lp = (C.c_void_p * 1)(lab.ctypes.data)
    ls = (C.c_size_t * 1)(4)
    rc = lib.pbd_candidate_mask(None, 1, _lib.ptr(rows, C.c_int), _lib.ptr(rows, C.c_int), None, 0, 0, lp, ls, 0, None, None, None, None)
    assert rc == -1                      # PBD_ERR_INVALID: no handle
    rc = lib.pbd_candidate_mask_device(None, 1, _lib.ptr(rows, C.c_int), _lib.ptr(rows, C.c_int), 0, 0, 0, lp, ls, 0, None, None, None,
                                       None, 0)
    assert rc == -1
    assert lib.pbd_part_poses(None, 0, None, None, None, None, None, None, None) == -1
    assert lib.pbd_part_poses_device(None, 0, 0, None, None, None, None, None, None, None) == -1
