"""Numpy yardsticks of the rest of the callers' PointCloudClusterer (include/PointCloudClusterer.hpp:53-293), as include/pbd.h
states them for pbd_boxes3d_camera and pbd_cluster_objects:

    PinholeCamera                                  image_geometry's PinholeCameraModel::projectPixelTo3dRay (ros/Node.cpp:210)
    PointCloudClusterer.computeBoundingBoxes       :53-153, after Candidate::boundingBox3D
    PointCloudClusterer.clusterObjects             :157-293 (plane removal stays with the caller)
    cloud_from_depth                               an organized float32 cloud back-projected from a float depth image

These run on the host, in numpy, and are what the device results are compared with bit for bit.  The device forms are
PartsBasedDetector.computeBoundingBoxes / .clusterObjects (detector.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

PARTS_LITERAL, PARTS_XY = 0, 1
RADIUS = np.float32(0.01)                     # setClusterTolerance(0.010) (:213), as the float PCL keeps
RADIUS2 = float(RADIUS) * float(RADIUS)       # (double)0.01f * (double)0.01f, exact
CELL_INV = np.float32(50.0)                   # 2 cm cells: 1 / edge


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
        ok = np.isfinite(p).all(axis=1) & (p >= g[0]).all(axis=1) & (p <= g[1]).all(axis=1)
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
        offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
        offs = [o for o in offs if o > (0, 0, 0)] + [(0, 0, 0)]          # each unordered cell pair once
        for dx, dy, dz in offs:
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
            e = d2.astype(np.float64) <= RADIUS2
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
        best = int(np.flatnonzero(size == size.max())[0])        # the largest; ties: the smallest first index
        members = np.nonzero(lab == best)[0]
        return centroid(P[members]), idx[members]

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
