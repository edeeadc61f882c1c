"""The numpy yardsticks of pbd_boxes3d_camera and pbd_cluster_objects (partsbaseddetector_amd/pointcloud.py), pinned on the
CPU against literal restatements of include/PointCloudClusterer.hpp:99-140 and of PCL's seed-queue clustering
(extractEuclideanClusters order, then the largest cluster, ties to the smallest first index)."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd.pointcloud import (PARTS_LITERAL, PARTS_XY, PinholeCamera, PointCloudClusterer as PCC, centroid,
                                               cloud_from_depth)

CAM = PinholeCamera(525.0, 520.0, 319.5, 239.5, 0.25, -0.5)
F = np.float32


def literal_edge(a, b):
    dx, dy, dz = F(a[0]) - F(b[0]), F(a[1]) - F(b[1]), F(a[2]) - F(b[2])
    d2 = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
    return float(d2) <= float(F(0.01)) * float(F(0.01))


def literal_cluster(cloud, box):
    """CropBox, then the seed-queue BFS of extractEuclideanClusters over the cropped indices, a brute-force radius search"""
    pts = cloud.reshape(-1, cloud.shape[-1])[:, :3]
    x, y, z, h, w, d = (float(v) for v in box)
    idx = []
    if w * h * d >= 1e-6:
        x, y, z = x - w * 0.1, y - h * 0.1, z - d * 0.1
        w, h, d = w * 1.2, h * 1.2, d * 1.2
        lo = [F(x), F(y), F(z)]
        hi = [F(x + w), F(y + h), F(z + d)]
        for i, p in enumerate(pts):
            if all(math.isfinite(float(v)) for v in p) and all(lo[k] <= p[k] <= hi[k] for k in range(3)):
                idx.append(i)
    m = len(idx)
    processed = [False] * m
    clusters = []
    for i in range(m):
        if processed[i]:
            continue
        q, k = [i], 0
        processed[i] = True
        while k < len(q):
            for j in range(m):
                if not processed[j] and literal_edge(pts[idx[q[k]]], pts[idx[j]]):
                    processed[j] = True
                    q.append(j)
            k += 1
        clusters.append(sorted(q))
    if not clusters:
        return np.full(3, np.nan, np.float32), []
    clusters.sort(key=lambda c: (-len(c), c[0]))
    best = [idx[j] for j in clusters[0]]
    s = [F(0), F(0), F(0)]
    for i in best:
        for k in range(3):
            s[k] = F(s[k] + pts[i][k])
    return np.array([s[k] / F(len(best)) for k in range(3)], np.float32), best


def same_f32(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def scene(rng, n, nan=True):
    """a few clumps of points 2-8 mm apart, duplicates, pairs on the radius, and non-finite points"""
    pts = []
    for _ in range(int(rng.integers(1, 5))):
        c = rng.uniform(-0.1, 0.1, 3)
        k = int(rng.integers(1, n))
        step = rng.uniform(0.002, 0.012)
        pts += list(c + np.cumsum(rng.normal(0, step, (k, 3)), axis=0))
    pts = np.array(pts, np.float32)
    if len(pts) > 2:
        pts = np.concatenate([pts, pts[rng.integers(0, len(pts), 3)]])               # duplicates
    # pairs whose distance is the radius give or take a few ulps, in either direction of rounding
    for t in range(4):
        a = pts[int(rng.integers(0, len(pts)))].copy()
        b = a.copy()
        b[t % 3] = np.nextafter(F(a[t % 3] + F(0.01)), F(np.inf if t & 1 else -np.inf))
        for _ in range(int(rng.integers(0, 3))):
            b[t % 3] = np.nextafter(b[t % 3], F(np.inf if t & 2 else -np.inf))
        pts = np.concatenate([pts, b[None]])
    if nan:
        bad = pts[:3].copy()
        bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
        pts = np.concatenate([pts, bad])
    return pts[rng.permutation(len(pts))]


def box_around(pts, rng):
    good = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = good.min(axis=0), good.max(axis=0)
    span = hi - lo
    lo = lo + span * rng.uniform(-0.1, 0.3, 3)
    hi = hi - span * rng.uniform(-0.1, 0.3, 3)
    return np.array([lo[0], lo[1], lo[2], hi[1] - lo[1], hi[0] - lo[0], hi[2] - lo[2]], np.float64)


@pytest.mark.parametrize("seed", range(30))
def test_cluster_yardstick_equals_literal_bfs(seed):
    rng = np.random.default_rng(seed)
    pts = scene(rng, 40)
    box = box_around(pts, rng)
    organized = seed % 2 == 0 and len(pts) % 2 == 0
    cloud = pts.reshape(2, -1, 3) if organized else pts                                  # odd seeds: an unorganized cloud
    want_c, want_i = literal_cluster(cloud, box)
    got_c, got_i = PCC.clusterObject(cloud, box)
    assert list(got_i) == want_i
    assert same_f32(got_c, want_c)


def test_radius_boundary_both_directions():
    """points placed at the radius give or take an ulp: the predicate, not the grid, decides"""
    r = F(0.01)
    for base in (F(0.0), F(0.3), F(-1.7), F(2.5)):
        for axis in range(3):
            for k in range(-3, 4):
                a = np.array([base, F(0.5), F(1.25)], np.float32)
                b = a.copy()
                v = F(a[axis] + r)
                for _ in range(abs(k)):
                    v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
                b[axis] = v
                pts = np.stack([a, b])
                lab = PCC.components(pts)
                assert (lab[1] == 0) == literal_edge(a, b), (base, axis, k)


def test_crop_faces_are_inside_and_gate():
    box = np.array([0.1, 0.2, 1.0, 0.3, 0.4, 0.5])
    lo, hi = PCC.cropBox(box)
    pts = np.array([lo, hi, [lo[0], hi[1], lo[2]], np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))], np.float32)
    assert list(PCC.crop(pts, box)) == [0, 1, 2]
    for empty in ([0, 0, 1, 0, 0, 0], [0, 0, 1, 0.1, 0.1, -0.2], [0, 0, 1, 0.01, 0.01, 0.009], [np.nan, 0, 1, 1, 1, 1]):
        c, ix = PCC.clusterObject(pts, empty)
        assert not len(ix) and np.isnan(c).all()
        want_c, want_i = literal_cluster(pts, empty)
        assert want_i == [] and np.isnan(want_c).all()


def test_size_tie_keeps_the_smallest_first_index():
    a = np.array([[0, 0, 1], [0.005, 0, 1]], np.float32)
    b = a + np.float32([0.5, 0, 0])
    pts = np.concatenate([b[:1], a, b[1:]])                # clusters {0, 3} and {1, 2}: the first index decides
    box = [-0.1, -0.1, 0.9, 0.2, 0.8, 0.2]
    c, ix = PCC.clusterObject(pts, box)
    assert list(ix) == [0, 3] == literal_cluster(pts, box)[1]


def test_grid_components_on_a_larger_cloud():
    rng = np.random.default_rng(5)
    pts = np.concatenate([c + rng.normal(0, 0.004, (150, 3)) for c in rng.uniform(0, 0.08, (4, 3))]).astype(np.float32)
    box = box_around(pts, rng)
    want_c, want_i = literal_cluster(pts, box)
    got_c, got_i = PCC.clusterObject(pts, box)
    assert list(got_i) == want_i and same_f32(got_c, want_c)


def test_centroid_is_the_ordered_fp32_sum():
    rng = np.random.default_rng(2)
    P = (rng.normal(0, 1, (1000, 3)) * np.array([1e3, 1, 1e-3])).astype(np.float32)
    s = [F(0)] * 3
    for p in P:
        s = [F(s[k] + p[k]) for k in range(3)]
    assert same_f32(centroid(P), [s[k] / F(len(P)) for k in range(3)])


# ---- part centres --------------------------------------------------------------------------------------------------------------
def literal_centres(parts, im_shape, depth, cam, mode):
    """a line-by-line restatement of PointCloudClusterer.hpp:99-140 (mode LITERAL) or its XY form"""
    rows, cols = im_shape
    out, dense = [], True
    for (x, y, w, h) in parts:
        x1, y1 = max(x, 0), max(y, 0)
        x2, y2 = min(x + w, cols), min(y + h, rows)
        x, y, w, h = (x1, y1, x2 - x1, y2 - y1) if x2 > x1 and y2 > y1 else (0, 0, 0, 0)
        cx, cy = x + int(w / 2), y + int(h / 2)
        avg = 0.0
        r0, c0 = (x, y) if mode == PARTS_LITERAL else (y, x)
        outside = False
        for row_it in range(r0, r0 + h):
            for col_it in range(c0, c0 + w):
                if row_it >= depth.shape[0] or col_it >= depth.shape[1]:
                    outside = True
                    continue
                avg += float(depth[row_it, col_it])
        if outside:
            p = [F(np.nan)] * 3
        else:
            if w * h != 0:
                avg /= w * h
            rx, ry = ((cx - cam.cx) - cam.tx) / cam.fx, ((cy - cam.cy) - cam.ty) / cam.fy
            p = [F(rx * avg), F(ry * avg), F(1.0 * avg)]
        if any(math.isnan(float(v)) for v in p):
            dense = False
        out.append(p)
    return np.array(out, np.float32), dense


@pytest.mark.parametrize("mode", [PARTS_LITERAL, PARTS_XY])
def test_part_centres_equal_the_line_by_line_loop(mode):
    rng = np.random.default_rng(11 + mode)
    im_shape = (48, 64)
    for dshape in ((48, 64), (30, 90), (64, 40)):                 # depth sizes other than the colour size too
        depth = rng.uniform(0.5, 3.0, dshape).astype(np.float32)
        depth[rng.random(dshape) < 0.05] = 0
        parts = [tuple(int(v) for v in (rng.integers(-10, 70), rng.integers(-10, 50), rng.integers(0, 30), rng.integers(0, 30)))
                 for _ in range(40)]
        parts += [(-20, -20, 5, 5), (70, 10, 5, 5), (0, 0, 0, 0), (40, 5, 10, 3), (5, 40, 3, 10)]   # empty, leaving the image
        want, wd = literal_centres(parts, im_shape, depth, CAM, mode)
        got, gd = PCC.partCentres(parts, im_shape, depth, CAM, mode)
        assert same_f32(got, want) and gd == wd


def test_empty_part_signed_zeros_and_nan_samples():
    depth = np.ones((10, 10), np.float32)
    got, dense = PCC.partCentres([(-5, -5, 2, 2)], (10, 10), depth, CAM)
    rx, ry = ((0 - CAM.cx) - CAM.tx) / CAM.fx, ((0 - CAM.cy) - CAM.ty) / CAM.fy
    assert same_f32(got[0], [F(rx * 0.0), F(ry * 0.0), F(0.0)]) and dense
    assert np.signbit(got[0, 0]) and np.signbit(got[0, 1]) and not np.signbit(got[0, 2])
    depth[2, 3] = np.nan
    got, dense = PCC.partCentres([(2, 1, 4, 4)], (10, 10), depth, CAM)   # literal rows 2.., columns 1..: holds (2, 3)
    assert np.isnan(got).all() and not dense
    got, dense = PCC.partCentres([(2, 1, 4, 4)], (10, 10), depth, CAM, PARTS_XY)   # XY rows 1..4, columns 2..5: holds it too
    assert np.isnan(got).all() and not dense


def test_camera_box_and_cloud_from_depth():
    cube = (100.0, 50.0, 1.5, 80.0, 40.0, 0.25)
    b = PCC.cameraBox(cube, CAM)
    tx, ty = ((100.0 - CAM.cx) - CAM.tx) / CAM.fx, ((50.0 - CAM.cy) - CAM.ty) / CAM.fy
    bx, by = ((140.0 - CAM.cx) - CAM.tx) / CAM.fx, ((130.0 - CAM.cy) - CAM.ty) / CAM.fy
    assert b == (tx * 1.5, ty * 1.5, 1.5, by * 1.75 - ty * 1.5, bx * 1.75 - tx * 1.5, 1.75 - 1.5)
    assert PCC.cameraBox((np.nan, 0, 0, 0, 0, 0), CAM) == (0.0,) * 6
    d = np.array([[1.0, 0.0], [np.nan, np.inf]], np.float32)
    c = cloud_from_depth(d, CAM)
    assert c.shape == (2, 2, 3) and c.dtype == np.float32
    assert same_f32(c[0, 0], [F(((0 - CAM.cx) - CAM.tx) / CAM.fx * 1.0), F(((0 - CAM.cy) - CAM.ty) / CAM.fy * 1.0), 1.0])
    assert np.isnan(c[0, 1]).all() and np.isnan(c[1]).all()


# ---- the clustering workspace (pbd_capi_post.hip: cluster_layout), host logic, no GPU needed -------------------------------------
def test_cluster_workspace_layout_near_the_crop_limit():
    """The bucket table, the scan partials and every carved piece fit their int / index ranges up to the largest accepted crop
    capacity (2^29), and a larger one is refused before anything is sized."""
    import ctypes as C
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pbd_debug_cluster_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 19)()
    for cap, maxpts, crop in ((1, 1, 0), (218, 640 * 480, 7456991), (16384, 1920 * 1080, (1 << 29) - 1), (64, 640 * 480, 1 << 29),
                              (3, 5, 1)):
        assert fn(cap, maxpts, crop, out) == 0, (cap, maxpts, crop)
        nchunks, units, tcap, nparts, total = out[0:5]
        sizes = list(out[5:19])
        assert nchunks == -(-maxpts // 1024) and units == cap * nchunks
        assert tcap & (tcap - 1) == 0 and tcap >= 2 * crop and tcap <= 2 ** 30 and (crop == 0 or tcap < 4 * crop or tcap == 2)
        assert tcap + 1 < 2 ** 31                                   # bucket indices, bstart[tcap] and the int the kernels take
        scan_tiles = max(-(-units // 1024), -(-tcap // 1024))
        assert nparts >= scan_tiles + 1                             # the partials of either scan and their total
        assert sizes[0] >= (units + 1) * 8 and sizes[1] == nparts * 8
        assert sizes[2:9] == [crop * 4, crop * 4, crop * 16, crop * 4, crop * 4, crop * 4, crop * 4]
        assert sizes[9] == sizes[10] == (tcap + 1) * 4 and sizes[11] == sizes[12] == cap * 8 and sizes[13] == 32
        assert total == sum(-(-b // 256) * 256 for b in sizes)
    for crop in ((1 << 29) + 1, 1 << 30, (1 << 31) - 1):
        assert fn(16, 640 * 480, crop, out) == -1
    assert fn(-1, 1, 1, out) == -1
