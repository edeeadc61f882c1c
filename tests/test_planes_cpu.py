"""The numpy yardstick of plane removal (pointcloud.PointCloudClusterer.organizedMultiplaneSegmentation) pinned against literal
restatements: a per-pixel normal loop, PCL's two-pass connected-component labelling with left and upper comparisons, and the two
refinement passes written as PCL writes them (nested loops, labels changed in place).  Also the pbd_remove_planes symbols and
the refusals that need no GPU.  No GPU is used here."""
import ctypes as C
import math

import numpy as np
import pytest

import planes_scenes as S
from partsbaseddetector_amd import pointcloud as pc
from partsbaseddetector_amd.pointcloud import PlaneParams, PointCloudClusterer as PCC

F = np.float32


def literal_normal(P, r, c, s=5, t=0.02):
    """the normal and d of pixel (r, c), one scalar operation at a time"""
    H, W = P.shape[:2]
    nan = (F(np.nan),) * 4
    if not (s + 1 <= r <= H - s - 2 and s + 1 <= c <= W - s - 2):
        return nan
    fin = lambda i, k: bool(np.isfinite(P[i, k]).all())
    for i in range(r - s, r + s + 1):
        for k in range(c - s, c + s + 1):
            if not fin(i, k):
                return nan
            z = P[i, k, 2]
            for a, b in ((i, k - 1), (i, k + 1), (i - 1, k), (i + 1, k)):
                if not fin(a, b) or abs(F(P[a, b, 2] - z)) > F(F(t) * z):
                    return nan
    sx = [F(0)] * 3
    sy = [F(0)] * 3
    for i in range(r - s, r + s + 1):
        rx = [F(0)] * 3
        ry = [F(0)] * 3
        for k in range(c - s, c + s + 1):
            for j in range(3):
                rx[j] = F(rx[j] + F(P[i, k + 1, j] - P[i, k - 1, j]))
                ry[j] = F(ry[j] + F(P[i + 1, k, j] - P[i - 1, k, j]))
        for j in range(3):
            sx[j] = F(sx[j] + rx[j])
            sy[j] = F(sy[j] + ry[j])
    area = F((2 * s + 1) ** 2)
    mx = [F(v / area) for v in sx]
    my = [F(v / area) for v in sy]
    n = [F(F(my[1] * mx[2]) - F(my[2] * mx[1])), F(F(my[2] * mx[0]) - F(my[0] * mx[2])), F(F(my[0] * mx[1]) - F(my[1] * mx[0]))]
    ln = F(np.sqrt(F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))))
    n = [F(v / ln) for v in n]
    p = P[r, c]
    dot = lambda: F(F(F(n[0] * p[0]) + F(n[1] * p[1])) + F(n[2] * p[2]))
    if dot() > 0:
        n = [-v for v in n]
    return n[0], n[1], n[2], dot()


def literal_segments(P, N, D, dist=0.02, angle=3.0 * math.pi / 180.0):
    """OrganizedConnectedComponentSegmentation's two passes: provisional labels from the left and upper neighbours with an
    equivalence table, then the raster relabelling (segments numbered by their first point); -1 for points that are not finite"""
    H, W = P.shape[:2]
    cos_thr = F(math.cos(angle))
    fin = np.isfinite(P).all(axis=2)
    lab = np.full((H, W), -1, np.int64)
    parent = []

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def join(p, q):
        if not fin[q]:
            return False
        z = P[p][2]
        near = abs(F(D[p] - D[q])) < F(F(dist) * F(z * z))
        dot = F(F(F(N[p][0] * N[q][0]) + F(N[p][1] * N[q][1])) + F(N[p][2] * N[q][2]))
        return bool(near and dot > cos_thr)

    for r in range(H):
        for c in range(W):
            if not fin[r, c]:
                continue
            got = [lab[q] for q in ((r, c - 1), (r - 1, c)) if q[0] >= 0 and q[1] >= 0 and join((r, c), q)]
            if not got:
                lab[r, c] = len(parent)
                parent.append(len(parent))
                continue
            roots = sorted({find(g) for g in got})
            lab[r, c] = roots[0]
            for g in roots[1:]:
                parent[g] = roots[0]
    first = {}
    out = np.full((H, W), -1, np.int64)
    for r in range(H):
        for c in range(W):
            if lab[r, c] >= 0:
                out[r, c] = first.setdefault(find(lab[r, c]), r * W + c)
    return out


def literal_refine(lab, P, planes, dist=0.02):
    """PCL's refine: the forward and backward raster passes, in place; lab holds -1 (not finite), -2 (no plane) or a plane"""
    lab = lab.copy()
    H, W = lab.shape

    def compare(cur, nb):
        cl, nl = lab[cur], lab[nb]
        if not (cl >= 0 and nl < 0):              # the current label is a plane's, the neighbour's is not
            return False
        a, b, c, d = planes[cl]
        x, y, z = P[nb]
        dd = F(F(F(F(a * x) + F(b * y)) + F(c * z)) + d)
        zc = P[cur][2]
        return bool(abs(dd) < F(F(dist) * F(zc * zc)))

    for r in range(H - 1):
        for c in range(W - 1):
            if lab[r, c] == -1 or lab[r, c + 1] == -1:
                continue
            if compare((r, c), (r, c + 1)):
                lab[r, c + 1] = lab[r, c]
            if lab[r + 1, c] == -1:
                continue
            if compare((r, c), (r + 1, c)):
                lab[r + 1, c] = lab[r, c]
    for r in range(H - 1, 0, -1):
        for c in range(W - 1, 0, -1):
            if lab[r, c] == -1 or lab[r, c - 1] == -1:
                continue
            if compare((r, c), (r, c - 1)):
                lab[r, c - 1] = lab[r, c]
            if lab[r - 1, c] == -1:
                continue
            if compare((r, c), (r - 1, c)):
                lab[r - 1, c] = lab[r, c]
    return lab


def scenes():
    return {"room": S.room(60, 80)[0], "tilted": S.tilted(48, 64)[0], "patches": S.patches()[0]}


def pre_refine(P, q=PlaneParams()):
    """the yardstick's normals, segments and working labels before refinement"""
    H, W = P.shape[:2]
    N, D = pc.plane_normals(P, q.smoothing_size // 2, q.depth_change_factor)
    root = pc.plane_segments(P, N, D, q.distance_threshold, q.angular_threshold)
    fin = np.isfinite(P).all(axis=2).ravel()
    size = np.bincount(root[fin], minlength=H * W)
    lab = np.where(fin, -2, -1)
    planes = []
    for r in np.nonzero((size > q.min_inliers) & fin & (root == np.arange(H * W)))[0]:
        coef, curv = pc.plane_fit(P, (root == r).reshape(H, W), int(size[r]))
        if curv < q.max_curvature:
            lab[root == r] = len(planes)
            planes.append(coef)
    return N, D, root, lab.reshape(H, W), np.array(planes, np.float32).reshape(-1, 4)


@pytest.mark.parametrize("name", ["room", "tilted", "patches"])
def test_normals_match_the_per_pixel_loop(name):
    P = scenes()[name]
    N, D = pc.plane_normals(P, 5, 0.02)
    H, W = P.shape[:2]
    rng = np.random.default_rng(3)
    pix = [(r, c) for r in range(H) for c in range(W) if r in (5, 6, H - 7, H - 6) or c in (5, 6, W - 7, W - 6)]
    pix += [tuple(v) for v in rng.integers(0, [H, W], size=(150, 2))]
    valid = 0
    for r, c in pix:
        want = np.array(literal_normal(P, r, c), np.float32)
        got = np.array([N[r, c, 0], N[r, c, 1], N[r, c, 2], D[r, c]], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or (np.isnan(got).all() and np.isnan(want).all()), (r, c)
        valid += not np.isnan(want).any()
    assert valid > 0


@pytest.mark.parametrize("name", ["room", "tilted", "patches"])
def test_segments_match_two_pass_labelling(name):
    P = scenes()[name]
    N, D = pc.plane_normals(P, 5, 0.02)
    got = pc.plane_segments(P, N, D, 0.02, 3.0 * math.pi / 180.0).reshape(P.shape[:2])
    want = literal_segments(P, N, D)
    fin = np.isfinite(P).all(axis=2)
    assert np.array_equal(got[fin], want[fin])
    assert len(np.unique(got[fin])) < fin.sum()      # something was joined


@pytest.mark.parametrize("name", ["room", "tilted", "patches"])
def test_refinement_matches_the_in_place_passes(name):
    P = scenes()[name]
    q = PlaneParams(min_inliers=200)                 # the small clouds keep the literal loops quick
    _, _, _, lab, planes = pre_refine(P, q)
    assert len(planes)
    want = literal_refine(lab, P, planes)
    got = pc.plane_refine_pass(lab, P, planes, 0.02)
    got = pc.plane_refine_pass(got[::-1, ::-1], P[::-1, ::-1], planes, 0.02)[::-1, ::-1]
    assert np.array_equal(got, want)
    assert (want >= 0).sum() > (lab >= 0).sum()      # the passes absorbed something
    _, kept, labels, planes2 = PCC.organizedMultiplaneSegmentation(P, q)
    assert np.array_equal(labels, np.where(want >= 0, want, -1)) and np.array_equal(planes2, planes)
    assert np.array_equal(kept, np.nonzero(want.ravel() < 0)[0])


def test_segment_of_1000_points_is_no_plane_and_1001_is():
    P = S.patches()[0]
    N, D, root, lab, planes = pre_refine(P, PlaneParams(refine=0))
    fin = np.isfinite(P).all(axis=2).ravel()
    sizes = sorted(np.bincount(root[fin]).tolist())[-2:]
    assert sizes == [1000, 1001]
    assert len(planes) == 1 and (lab >= 0).sum() == 1001
    _, _, labels, _ = PCC.organizedMultiplaneSegmentation(P, PlaneParams(refine=0))
    assert (labels >= 0).sum() == 1001


def test_curvature_either_side_of_the_limit():
    for radius, planar in ((7.0, False), (7.5, True)):
        P = S.bent(60, 80, radius)[0]
        N, D = pc.plane_normals(P, 5, 0.02)
        root = pc.plane_segments(P, N, D, 0.02, 3.0 * math.pi / 180.0)
        size = np.bincount(root)
        r = int(size.argmax())
        assert size[r] > 3000                          # one segment
        _, curv = pc.plane_fit(P, (root == r).reshape(P.shape[:2]), int(size[r]))
        assert 0.0009 < curv < 0.0011 and (curv < 0.001) == planar
        assert len(PCC.organizedMultiplaneSegmentation(P)[3]) == int(planar)


def test_jacobi_eigenpair():
    A = [[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 0.01]]
    B = [row[:] for row in A]
    V = pc.jacobi3(B)
    w, v = np.linalg.eigh(np.array(A))
    k = int(np.argmin([B[i][i] for i in range(3)]))
    assert abs(B[k][k] - w[0]) < 1e-12
    assert abs(abs(np.dot(np.array(V)[:, k], v[:, 0])) - 1.0) < 1e-12


def test_output_is_the_complement_in_index_order():
    P = S.room(60, 80)[0]
    cloud, kept, labels, planes = PCC.organizedMultiplaneSegmentation(P, PlaneParams(min_inliers=200))
    assert len(planes) and (labels >= 0).any()
    flat = P.reshape(-1, 3)
    assert np.array_equal(kept, np.nonzero(labels.ravel() < 0)[0])
    assert np.array_equal(cloud.view(np.uint32), flat[kept].view(np.uint32))
    assert np.isnan(cloud).any()                     # NaN points stay in the reduced cloud


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from partsbaseddetector_amd import build, _lib
    build.build_hip()
    return _lib.load()


def test_symbols_and_null_handle_refusal(lib):
    from partsbaseddetector_amd import _lib
    assert hasattr(lib, "pbd_remove_planes") and hasattr(lib, "pbd_remove_planes_device")
    assert "pbd_remove_planes" in _lib.SYMBOLS and "pbd_remove_planes_device" in _lib.SYMBOLS
    cloud = np.zeros((4, 4, 3), np.float32)
    descs = _lib.cloud_array([(cloud.ctypes.data, 4, 4, 12, 48)])
    out = np.zeros(64, np.float32)
    need = C.c_int()
    rc = lib.pbd_remove_planes(None, 1, descs, None, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, None,
                               out.ctypes.data, 0, C.byref(need))
    assert rc == -1                      # PBD_ERR_INVALID: no handle
    rc = lib.pbd_remove_planes_device(None, 1, descs, None, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1                      # PBD_ERR_INVALID: no handle


def test_plane_params_struct_matches_the_defaults():
    from partsbaseddetector_amd import _lib
    p = _lib.plane_params(PlaneParams()).contents
    assert (p.smoothing_size, p.min_inliers, p.refine) == (10, 1000, 1)
    assert p.angular_threshold == 3.0 * math.pi / 180.0 and p.max_curvature == 0.001
    assert F(p.distance_threshold) == F(0.02) and F(p.depth_change_factor) == F(0.02)
    assert _lib.plane_params(None) is None
    assert C.sizeof(_lib.CPlaneParams) == 40
