"""Numpy yardsticks of the rest of the callers' PointCloudClusterer (include/PointCloudClusterer.hpp:53-293), as include/pbd.h
states them for pbd_boxes3d_camera and pbd_cluster_objects:

    PinholeCamera                                  image_geometry's PinholeCameraModel::projectPixelTo3dRay (ros/Node.cpp:210)
    PointCloudClusterer.computeBoundingBoxes       :53-153, after Candidate::boundingBox3D
    PointCloudClusterer.clusterObjects             :157-293, on the full cloud or the reduced cloud of plane removal
    PointCloudClusterer.organizedMultiplaneSegmentation  :294-336, as include/pbd.h states it for pbd_remove_planes
    cloud_from_depth                               an organized float32 cloud back-projected from a float depth image

These run on the host, in numpy, and are what the device results are compared with bit for bit.  The device forms are
PartsBasedDetector.computeBoundingBoxes / .clusterObjects / .removePlanes (detector.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

PARTS_LITERAL, PARTS_XY = 0, 1
RADIUS = np.float32(0.01)                     # setClusterTolerance(0.010) (:213), as the float PCL keeps
RADIUS2 = float(RADIUS) * float(RADIUS)       # (double)0.01f * (double)0.01f, exact
CELL_INV = np.float32(50.0)                   # 2 cm cells: 1 / edge


@dataclass(frozen=True)
class PlaneParams:
    """pbd_plane_params; the defaults are the reference's call (PCL's defaults, include/PointCloudClusterer.hpp:294-336)"""
    smoothing_size: int = 10
    depth_change_factor: float = 0.02
    distance_threshold: float = 0.02
    angular_threshold: float = 3.0 * math.pi / 180.0
    max_curvature: float = 0.001
    min_inliers: int = 1000
    refine: int = 1


JACOBI_SWEEPS = 8


# ---- the contract's comparisons and choices, each stated once.  The yardsticks below call them by name, so a test can swap a
# single one (tests/test_cloud_hard_cpu.py) and show that some input notices; none of them holds arithmetic of its own.
def edge_tolerance(t_centre, t_neighbour):
    """the depth-edge test |z(q) - z(p)| > depth_change * z compares with the z of the centre p"""
    return t_centre


def join_depth(z_current, z_neighbour):
    """the join threshold dist * z * z takes the z of the current point"""
    return z_current


def absorb_depth(z_from, z_absorbed):
    """the absorb threshold dist * z * z takes the z of the neighbour the plane comes from"""
    return z_from


def join_near(distance, threshold):
    """the join's distance test is strict"""
    return distance < threshold


def absorb_near(distance, threshold):
    """the absorb's distance test is strict"""
    return distance < threshold


def parallel(dot, cos_thr):
    """the angular test is strict"""
    return dot > cos_thr


def refine_upper_column(c, W):
    """the last column takes no label from above"""
    return c <= W - 2


def refine_upper_right(fin, r, c):
    """taking a label from above needs (r-1, c+1) finite (callers hold c <= W-2 unless refine_upper_column is changed)"""
    return fin[r - 1, np.minimum(c + 1, fin.shape[1] - 1)]


def refine_left_row(r, H):
    """the last row takes no label from the left"""
    return r <= H - 2


REFINE_ORDER = ("upper", "left")              # a point both neighbours would absorb takes the upper one's plane


def moment_total(v):
    """one moment of a segment: each row left to right from 0, then the row sums top to bottom from 0 (v: (rows, cols) doubles)"""
    rows = np.add.accumulate(np.concatenate([np.zeros((v.shape[0], 1)), v], axis=1), axis=1)[:, -1]
    return float(np.add.accumulate(np.concatenate([[0.0], rows]))[-1])


def inside(p, lo, hi):
    """the faces of the crop box are inside"""
    return (p >= lo).all(axis=1) & (p <= hi).all(axis=1)


def within_radius(d2):
    """a pair at the radius exactly is an edge"""
    return d2.astype(np.float64) <= RADIUS2


def neighbour_cells():
    """the 27 cells around a point's own, as 13 directions, their opposites implied (each unordered pair of cells once), and
    the cell itself"""
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
    return [o for o in offs if o > (0, 0, 0)] + [(0, 0, 0)]


def largest(size):
    """the largest component; ties: the smallest first index"""
    return int(np.flatnonzero(size == size.max())[0])


@dataclass(frozen=True)
class PinholeCamera:
    fx: float
    fy: float
    cx: float
    cy: float
    tx: float = 0.0
    ty: float = 0.0

    def projectPixelTo3dRay(self, u, v):
        """(((u - cx) - tx) / fx, ((v - cy) - ty) / fy, 1.0) in double (numpy broadcasting)"""
        return ((np.float64(u) - self.cx) - self.tx) / self.fx, ((np.float64(v) - self.cy) - self.ty) / self.fy, 1.0


def cloud_from_depth(depth_m: np.ndarray, camera: PinholeCamera) -> np.ndarray:
    """(rows, cols, 3) float32 organized cloud: pixel (r, c) -> ray(c, r) * d, rounded to float; NaN where d is 0, NaN or +-Inf"""
    d = np.asarray(depth_m, np.float64)
    rows, cols = d.shape
    rx, ry, _ = camera.projectPixelTo3dRay(np.arange(cols, dtype=np.float64)[None, :], np.arange(rows, dtype=np.float64)[:, None])
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([np.broadcast_to(rx * d, d.shape), np.broadcast_to(ry * d, d.shape), d], axis=-1).astype(np.float32)
    out[(d == 0) | ~np.isfinite(d)] = np.nan
    return out


def _rect_and(x, y, w, h, cols, rows):
    x1, y1 = max(x, 0), max(y, 0)
    w, h = min(x + w, cols) - x1, min(y + h, rows) - y1
    return (x1, y1, w, h) if w > 0 and h > 0 else (0, 0, 0, 0)


def _xyz(cloud: np.ndarray) -> np.ndarray:
    """(N, 3) float32 of a cloud given as (rows, cols, k) or (N, k), k >= 3: the first three floats of every point"""
    c = np.asarray(cloud)
    if c.dtype != np.float32:
        raise TypeError("clouds are float32")
    return c.reshape(-1, c.shape[-1])[:, :3]


class PointCloudClusterer:
    """The two steps the ECTO cell and the ROS node run after detection and suppression."""

    @staticmethod
    def cameraBox(cube, camera: PinholeCamera) -> Tuple[float, ...]:
        """Rect3d(tl, br) of a Candidate::boundingBox3D cube (:143-148); (0,)*6 when the cube holds a NaN (:80-81)"""
        cube = [float(v) for v in cube]
        if any(np.isnan(v) for v in cube):
            return (0.0,) * 6
        x, y, z, h, w, d = cube
        tx, ty, _ = camera.projectPixelTo3dRay(x, y)
        bx, by, _ = camera.projectPixelTo3dRay(x + w, y + h)
        z1 = z + d
        tl = (float(tx * z), float(ty * z), 1.0 * z)
        br = (float(bx * z1), float(by * z1), 1.0 * z1)
        return tl[0], tl[1], tl[2], br[1] - tl[1], br[0] - tl[0], br[2] - tl[2]

    @staticmethod
    def partCentres(parts, im_shape, depth: np.ndarray, camera: PinholeCamera, parts_mode: int = PARTS_LITERAL):
        """(nparts, 3) float32 centres of the parts (:99-140) and the dense flag.  LITERAL: rows x.., columns y.. (the reference's
        transposed loop); XY: rows y.., columns x...  A non-empty part whose samples leave the depth image: NaN x3."""
        rows, cols = int(im_shape[0]), int(im_shape[1])
        drows, dcols = depth.shape
        out = np.zeros((len(parts), 3), np.float32)
        for j, q in enumerate(parts):
            x, y, w, h = _rect_and(*(int(v) for v in q), cols, rows)
            u, v = x + w // 2, y + h // 2
            r0, c0 = (x, y) if parts_mode == PARTS_LITERAL else (y, x)
            if w * h != 0 and (r0 + h > drows or c0 + w > dcols):
                out[j] = np.nan
                continue
            samples = depth[r0:r0 + h, c0:c0 + w].astype(np.float64).ravel()
            s = float(np.cumsum(samples)[-1]) if samples.size else 0.0     # sequential, row-major
            if w * h != 0:
                s = s / float(w * h)
            rx, ry, _ = camera.projectPixelTo3dRay(u, v)
            with np.errstate(invalid="ignore", over="ignore"):
                out[j] = np.array([rx * s, ry * s, 1.0 * s], np.float64).astype(np.float32)
        dense = not np.isnan(out).any()
        return out, dense

    @staticmethod
    def computeBoundingBoxes(candidates, im_shapes, depths, cameras, parts_mode: int = PARTS_LITERAL, max_parts: int = None,
                             cubes=None):
        """Every candidate's camera box and part centres: (boxes (n, 6) float64, centres (n, max_parts, 3) float32 (zero past a
        record's ncentres), ncentres (n,) int32, dense (n,) int32).  im_shapes / depths / cameras are indexed by c.frame;
        `cubes` (n, 6) may give the boundingBox3D results already computed."""
        n = len(candidates)
        mp = max_parts or max([len(c.parts) for c in candidates] + [1])
        boxes = np.zeros((n, 6))
        centres = np.zeros((n, mp, 3), np.float32)
        ncent = np.zeros(n, np.int32)
        dense = np.ones(n, np.int32)
        for i, c in enumerate(candidates):
            f = c.frame
            cube = cubes[i] if cubes is not None else c.boundingBox3D(im_shapes[f], depths[f])
            if np.isnan(np.asarray(cube, np.float64)).any():
                continue
            boxes[i] = PointCloudClusterer.cameraBox(cube, cameras[f])
            cen, dn = PointCloudClusterer.partCentres(c.parts, im_shapes[f], depths[f], cameras[f], parts_mode)
            centres[i, :len(cen)] = cen
            ncent[i] = len(cen)
            dense[i] = int(dn)
        return boxes, centres, ncent, dense

    @staticmethod
    def cropBox(box) -> Tuple[np.ndarray, np.ndarray]:
        """the gate and expansion of :190-206: (min, max) float32[3], or None when the box has no points"""
        x, y, z, h, w, d = (float(v) for v in box)
        if not (w * h * d >= 1e-6):
            return None
        x, y, z = x - w * 0.1, y - h * 0.1, z - d * 0.1
        w, h, d = w * 1.2, h * 1.2, d * 1.2
        return np.array([x, y, z], np.float32), np.array([x + w, y + h, z + d], np.float32)

    @staticmethod
    def crop(cloud, box) -> np.ndarray:
        """pcl::CropBox on a cloud taken as not dense: ascending indices of the finite points inside the expanded box"""
        g = PointCloudClusterer.cropBox(box)
        if g is None:
            return np.zeros(0, np.int64)
        p = _xyz(cloud)
        ok = np.isfinite(p).all(axis=1) & inside(p, g[0], g[1])
        return np.nonzero(ok)[0]

    @staticmethod
    def components(P: np.ndarray) -> np.ndarray:
        """label of every point of P (m, 3) float32 = the smallest index of its connected component under the edge predicate.
        A grid of 2 cm cells prunes the pairs; label propagation (min over edges, then pointer jumping) until nothing changes."""
        m = len(P)
        lab = np.arange(m)
        if m < 2:
            return lab
        cell = np.floor(P * CELL_INV).astype(np.int64)
        cell -= cell.min(axis=0)
        span = cell.max(axis=0) + 3
        key = ((cell[:, 0] + 1) * span[1] + (cell[:, 1] + 1)) * span[2] + (cell[:, 2] + 1)
        order = np.argsort(key, kind="stable")
        skey = key[order]
        ukey, ustart, ucount = np.unique(skey, return_index=True, return_counts=True)
        ea, eb = [], []
        for dx, dy, dz in neighbour_cells():                             # each unordered cell pair once
            nk = ukey + (dx * span[1] + dy) * span[2] + dz
            pos = np.searchsorted(ukey, nk)
            pos = np.minimum(pos, len(ukey) - 1)
            hit = ukey[pos] == nk
            ca, cb = np.nonzero(hit)[0], pos[hit]                           # cell pairs (a, b)
            if not len(ca):
                continue
            na, nb = ucount[ca], ucount[cb]
            tot = na * nb
            # every (point of a, point of b) pair
            pa_cell = np.repeat(np.arange(len(ca)), tot)
            within = np.arange(tot.sum()) - np.repeat(np.cumsum(tot) - tot, tot)
            ia = ustart[ca][pa_cell] + within // nb[pa_cell]
            ib = ustart[cb][pa_cell] + within % nb[pa_cell]
            a, b = order[ia], order[ib]
            if (dx, dy, dz) == (0, 0, 0):
                keep = a < b
                a, b = a[keep], b[keep]
            dd = P[a] - P[b]
            d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            e = within_radius(d2)
            ea.append(a[e])
            eb.append(b[e])
        if not ea:
            return lab
        ea, eb = np.concatenate(ea), np.concatenate(eb)
        while True:
            prev = lab.copy()
            la, lb = lab[ea], lab[eb]
            mn = np.minimum(la, lb)
            for t in (ea, eb, la, lb):                          # the endpoints and their labels' points hook to the smaller
                np.minimum.at(lab, t, mn)
            while True:
                nxt = lab[lab]
                if np.array_equal(nxt, lab):
                    break
                lab = nxt
            if np.array_equal(lab, prev):
                return lab

    @staticmethod
    def edgeCandidates(P: np.ndarray) -> int:
        """pairs j < i within the 27 neighbouring 2 cm cells (what the device's grid hands the exact predicate, before hash
        collisions)"""
        if len(P) < 2:
            return 0
        cell = np.floor(P * CELL_INV).astype(np.int64)
        cell -= cell.min(axis=0)
        span = cell.max(axis=0) + 3
        key = ((cell[:, 0] + 1) * span[1] + (cell[:, 1] + 1)) * span[2] + (cell[:, 2] + 1)
        ukey, count = np.unique(key, return_counts=True)
        total = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    nk = ukey + (dx * span[1] + dy) * span[2] + dz
                    pos = np.minimum(np.searchsorted(ukey, nk), len(ukey) - 1)
                    hit = ukey[pos] == nk
                    total += int((count[hit] * count[pos[hit]]).sum())
        return (total - len(P)) // 2

    @staticmethod
    def clusterObject(cloud, box) -> Tuple[np.ndarray, np.ndarray]:
        """one box: (centre float32[3] (NaN x3 without a cluster), ascending point indices of the kept cluster)"""
        idx = PointCloudClusterer.crop(cloud, box)
        if not len(idx):
            return np.full(3, np.nan, np.float32), idx
        P = _xyz(cloud)[idx]
        lab = PointCloudClusterer.components(P)
        size = np.bincount(lab, minlength=len(P))
        best = largest(size)
        members = np.nonzero(lab == best)[0]
        return centroid(P[members]), idx[members]

    @staticmethod
    def organizedMultiplaneSegmentation(cloud, params: PlaneParams = None):
        """(cloud_no_planes (k, 3) float32, kept (k,) int64 original indices, labels (rows, cols) int32 (plane index or -1),
        planes (n, 4) float32 {a, b, c, d}) of an organized cloud (rows, cols, >= 3) float32; the inlier counts are
        np.bincount(labels[labels >= 0], minlength=n).  Follows include/pbd.h's contract op by op."""
        q = params or PlaneParams()
        c = np.asarray(cloud)
        if c.dtype != np.float32 or c.ndim != 3 or c.shape[2] < 3 or c.shape[0] < 2 or c.shape[1] < 2:
            raise ValueError("an organized float32 cloud (rows >= 2, cols >= 2, >= 3 floats per point)")
        P = np.ascontiguousarray(c[:, :, :3])
        H, W = P.shape[:2]
        fin = np.isfinite(P).all(axis=2)
        n, d = plane_normals(P, q.smoothing_size // 2, q.depth_change_factor)
        root = plane_segments(P, n, d, q.distance_threshold, q.angular_threshold)
        size = np.bincount(root[fin.ravel()], minlength=H * W)
        cand = np.nonzero((size > q.min_inliers) & fin.ravel() & (root == np.arange(H * W)))[0]
        planes = []
        lab = np.where(fin, -2, -1).astype(np.int64).ravel()
        for r in cand:
            coef, curv = plane_fit(P, (root == r).reshape(H, W), int(size[r]))
            if curv < q.max_curvature:
                lab[(root == r)] = len(planes)
                planes.append(coef)
        planes = np.array(planes, np.float32).reshape(-1, 4)
        lab = lab.reshape(H, W)
        if q.refine and len(planes):
            lab = plane_refine(lab, P, planes, q.distance_threshold)
        lab = np.ascontiguousarray(lab)
        kept = np.nonzero(lab.ravel() < 0)[0]
        labels = np.where(lab >= 0, lab, -1).astype(np.int32)
        return P.reshape(-1, 3)[kept].copy(), kept.astype(np.int64), labels, planes

    @staticmethod
    def clusterObjects(clouds, boxes, frames) -> Tuple[np.ndarray, List[np.ndarray]]:
        """every box: (centres (n, 3) float32, [ascending point indices of the kept cluster]); box i is cropped from
        clouds[frames[i]]"""
        n = len(boxes)
        centres = np.zeros((n, 3), np.float32)
        out = []
        for i in range(n):
            centres[i], ix = PointCloudClusterer.clusterObject(clouds[int(frames[i])], boxes[i])
            out.append(ix.astype(np.int64))
        return centres, out


def centroid(P: np.ndarray) -> np.ndarray:
    """pcl::compute3DCentroid of finite points: three sequential fp32 sums, each / (float)count"""
    s = np.cumsum(np.asarray(P, np.float32), axis=0, dtype=np.float32)[-1]
    return (s / np.float32(len(P))).astype(np.float32)


def gather(cloud, indices) -> np.ndarray:
    """the points of `indices` (ExtractIndices::filter), (k, 3) float32"""
    return _xyz(cloud)[np.asarray(indices, np.int64)]


# ---- plane removal (include/pbd.h, pbd_remove_planes); every float32 / float64 operation rounded on its own, in order
_F = np.float32


def plane_normals(P: np.ndarray, s: int, depth_change: float):
    """(normals (rows, cols, 3) float32, d (rows, cols) float32): NaN off the valid window or where it holds a depth edge"""
    H, W = P.shape[:2]
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    fin = np.isfinite(P).all(axis=2)
    edge = np.ones((H, W), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        t = _F(depth_change) * z
        e = ~fin[1:-1, 1:-1]
        zc, tc = z[1:-1, 1:-1], t[1:-1, 1:-1]
        for sl in ((slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)), (slice(0, -2), slice(1, -1)),
                   (slice(2, None), slice(1, -1))):
            e |= ~fin[sl] | (np.abs(z[sl] - zc) > edge_tolerance(tc, t[sl]))
        edge[1:-1, 1:-1] = e
        dx = np.full_like(P, np.nan)
        dy = np.full_like(P, np.nan)
        dx[:, 1:-1] = P[:, 2:] - P[:, :-2]
        dy[1:-1] = P[2:] - P[:-2]
        N = np.full((H, W, 3), np.nan, np.float32)
        D = np.full((H, W), np.nan, np.float32)
        r0, r1, c0, c1 = s + 1, H - s - 1, s + 1, W - s - 1          # valid centres: [r0, r1) x [c0, c1)
        if r1 <= r0 or c1 <= c0:
            return N, D
        # row sums over columns c-s .. c+s for rows 1 .. H-2, left to right from 0
        rsx = np.zeros((H - 2, c1 - c0, 3), np.float32)
        rsy = np.zeros((H - 2, c1 - c0, 3), np.float32)
        redge = np.zeros((H - 2, c1 - c0), bool)
        for k in range(-s, s + 1):
            rsx = rsx + dx[1:-1, c0 + k:c1 + k]
            rsy = rsy + dy[1:-1, c0 + k:c1 + k]
            redge |= edge[1:-1, c0 + k:c1 + k]
        # the row sums of rows r-s .. r+s, top to bottom from 0
        sx = np.zeros((r1 - r0, c1 - c0, 3), np.float32)
        sy = np.zeros((r1 - r0, c1 - c0, 3), np.float32)
        wedge = np.zeros((r1 - r0, c1 - c0), bool)
        for k in range(-s, s + 1):
            sx = sx + rsx[r0 - 1 + k:r1 - 1 + k]
            sy = sy + rsy[r0 - 1 + k:r1 - 1 + k]
            wedge |= redge[r0 - 1 + k:r1 - 1 + k]
        area = _F((2 * s + 1) * (2 * s + 1))
        mx, my = sx / area, sy / area
        nx = my[..., 1] * mx[..., 2] - my[..., 2] * mx[..., 1]
        ny = my[..., 2] * mx[..., 0] - my[..., 0] * mx[..., 2]
        nz = my[..., 0] * mx[..., 1] - my[..., 1] * mx[..., 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        px, py, pz = x[r0:r1, c0:c1], y[r0:r1, c0:c1], z[r0:r1, c0:c1]
        flip = ((nx * px + ny * py) + nz * pz) > 0
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
        dd = (nx * px + ny * py) + nz * pz
        nan = _F(np.nan)
        N[r0:r1, c0:c1] = np.where(wedge[..., None], nan, np.stack([nx, ny, nz], axis=-1))
        D[r0:r1, c0:c1] = np.where(wedge, nan, dd)
    return N, D


def plane_join(zp, np_, dp, fq, nq, dq, dist: float, cos_thr, zq=None):
    """PlaneCoefficientComparator(p, q): q finite, |d(p) - d(q)| < dist * (z(p) * z(p)), n(p) . n(q) > cos_thr (arrays)"""
    with np.errstate(invalid="ignore", over="ignore"):
        zt = join_depth(zp, zq)
        near = join_near(np.abs(dp - dq), _F(dist) * (zt * zt))
        dot = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
        return fq & near & parallel(dot, cos_thr)


def plane_segments(P, N, D, dist: float, angle: float) -> np.ndarray:
    """the segment of every point as the smallest point index of its component (rows * cols,) int64 (non-finite: itself)"""
    H, W = P.shape[:2]
    fin = np.isfinite(P).all(axis=2)
    cos_thr = _F(math.cos(angle))
    z = P[..., 2]
    idx = np.arange(H * W).reshape(H, W)
    left = fin[:, 1:] & plane_join(z[:, 1:], N[:, 1:], D[:, 1:], fin[:, :-1], N[:, :-1], D[:, :-1], dist, cos_thr, z[:, :-1])
    up = fin[1:] & plane_join(z[1:], N[1:], D[1:], fin[:-1], N[:-1], D[:-1], dist, cos_thr, z[:-1])
    ea = np.concatenate([idx[:, 1:][left], idx[1:][up]])
    eb = np.concatenate([idx[:, :-1][left], idx[:-1][up]])
    return min_label_components(H * W, ea, eb)


def min_label_components(n: int, ea: np.ndarray, eb: np.ndarray) -> np.ndarray:
    """the smallest node of every node's connected component (edges ea[i] - eb[i])"""
    lab = np.arange(n)
    if not len(ea):
        return lab
    while True:
        prev = lab.copy()
        la, lb = lab[ea], lab[eb]
        mn = np.minimum(la, lb)
        for t in (ea, eb, la, lb):
            np.minimum.at(lab, t, mn)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, prev):
            return lab


def jacobi3(A):
    """cyclic Jacobi sweeps on a symmetric 3x3 (lists of Python floats, modified in place); returns V"""
    V = [[1.0 if i == k else 0.0 for k in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(3):
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return V


def plane_fit(P, mask, count: int):
    """(coefficients float32[4], curvature) of the points of `mask` (rows, cols): moments per row left to right, rows top to
    bottom, the Jacobi eigenpair"""
    x, y, z = (np.where(mask, P[..., k].astype(np.float64), 0.0) for k in range(3))
    vals = (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)
    tot = [moment_total(v) for v in vals]
    n = float(count)
    m = [t / n for t in tot]
    xx, xy, xz = m[3] - m[0] * m[0], m[4] - m[0] * m[1], m[5] - m[0] * m[2]
    yy, yz, zz = m[6] - m[1] * m[1], m[7] - m[1] * m[2], m[8] - m[2] * m[2]
    A = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    V = jacobi3(A)
    k = 0
    if A[1][1] < A[k][k]:
        k = 1
    if A[2][2] < A[k][k]:
        k = 2
    tr = (xx + yy) + zz
    curv = _ieee_div(A[k][k], tr)
    a, b, c = V[0][k], V[1][k], V[2][k]
    d = -((a * m[0] + b * m[1]) + c * m[2])
    if ((-m[0]) * a + (-m[1]) * b) + (-m[2]) * c < 0.0:
        a, b, c, d = -a, -b, -c, -d
    return np.array([a, b, c, d], np.float64).astype(np.float32), curv


def _ieee_div(a: float, b: float) -> float:
    """a / b with IEEE semantics for b == 0"""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def plane_absorb(coef, pts, zc, dist: float):
    """|((a x + b y) + c z) + d| < dist * (zc * zc) in float32 (coef (k, 4), pts (k, 3))"""
    with np.errstate(invalid="ignore", over="ignore"):
        dd = ((coef[:, 0] * pts[:, 0] + coef[:, 1] * pts[:, 1]) + coef[:, 2] * pts[:, 2]) + coef[:, 3]
        zt = absorb_depth(zc, pts[:, 2])
        return absorb_near(np.abs(dd), _F(dist) * (zt * zt))


def plane_refine(lab, P, planes, dist: float) -> np.ndarray:
    """the forward pass, then the backward pass: the forward pass on the image turned by 180 degrees"""
    lab = plane_refine_pass(lab, P, planes, dist)
    return plane_refine_pass(lab[::-1, ::-1], P[::-1, ::-1], planes, dist)[::-1, ::-1]


def plane_refine_pass(lab, P, planes, dist: float) -> np.ndarray:
    """one forward refinement pass (include/pbd.h's recurrence, one anti-diagonal at a time); labels -1 / -2 / plane index"""
    H, W = lab.shape
    o = np.array(lab, np.int64)
    F = o.copy()
    fin = np.isfinite(P).all(axis=2)
    for t in range(H + W - 1):
        r = np.arange(max(0, t - W + 1), min(H - 1, t) + 1)
        c = t - r
        m = o[r, c].copy()
        for step in REFINE_ORDER:
            if step == "upper":
                sel = (r >= 1) & refine_upper_column(c, W) & (m == -2)
                dr, dc = 1, 0
            else:
                sel = (c >= 1) & refine_left_row(r, H) & (m == -2)
                dr, dc = 0, 1
            if not sel.any():
                continue
            rs, cs = r[sel], c[sel]
            src = F[rs - dr, cs - dc]
            ok = src >= 0
            if step == "upper":
                ok &= refine_upper_right(fin, rs, cs)
            ok[ok] = plane_absorb(planes[src[ok]], P[rs[ok], cs[ok]], P[rs[ok] - dr, cs[ok] - dc, 2], dist)
            mm = m[sel]
            mm[ok] = src[ok]
            m[sel] = mm
        F[r, c] = m
    return F
