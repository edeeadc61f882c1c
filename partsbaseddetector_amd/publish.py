"""numpy yardsticks of the ROS node's two remaining products (include/pbd.h states both contracts):

    candidate_mask / masked_image   Candidate::mask (include/Candidate.hpp:306-331) and `rgb & (mask != 0)` (ros/Messages.cpp:157-174)
    part_poses                      messagePoses (ros/Messages.cpp:187-234): centroid and eigen-frame of each part-centre cloud

The device forms (pbd_candidate_mask*, pbd_part_poses*) equal these bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from .pointcloud import jacobi3


def record_boxes(records: np.ndarray) -> np.ndarray:
    """boundingBox() of every record (n, stride): the hull of its parts under cv::Rect operator|, (n, 4) int64 (x, y, w, h)"""
    rec = np.asarray(records, np.int64)
    rec = rec.reshape(len(rec), -1) if rec.size else rec.reshape(0, 8)
    out = np.zeros((len(rec), 4), np.int64)
    for i, r in enumerate(rec):
        x, y, w, h = (int(v) for v in r[8:12])
        for j in range(int(r[6])):
            bx, by, bw, bh = (int(v) for v in r[8 + 4 * j:12 + 4 * j])
            if w <= 0 or h <= 0:
                x, y, w, h = bx, by, bw, bh
            elif bw > 0 and bh > 0:
                x1, y1 = min(x, bx), min(y, by)
                w, h = max(x + w, bx + bw) - x1, max(y + h, by + bh) - y1
                x, y = x1, y1
        out[i] = (x, y, w, h)
    return out


def candidate_mask(im_shape, boxes) -> np.ndarray:
    """Candidate::mask: uint8 (rows, cols) labels of the boxes (x, y, w, h) in list order.  A pixel's label is min(1 + n, 255) for
    the first box n that covers it (each box & Rect(0, 0, cols, rows)), 0 where none does.  Painting the boxes from the last to the
    first, each overwriting, leaves every pixel the first box that covers it."""
    rows, cols = int(im_shape[0]), int(im_shape[1])
    mask = np.zeros((rows, cols), np.uint8)
    for n in range(len(boxes) - 1, -1, -1):
        x, y, w, h = (int(v) for v in boxes[n])
        x1, y1, x2, y2 = max(x, 0), max(y, 0), min(x + w, cols), min(y + h, rows)
        if w <= 0 or h <= 0 or x2 <= x1 or y2 <= y1:
            continue
        mask[y1:y2, x1:x2] = min(n + 1, 255)
    return mask


def frame_masks(im_shapes, records: np.ndarray, frame_offset: int = 0):
    """candidate_mask of each frame index f (im_shapes[f] = (rows, cols)) over the records (n, stride) whose `frame` - frame_offset
    is f, in list order (the records grouped by ascending frame, as pbd_candidate_mask requires)"""
    rec = np.asarray(records, np.int32)
    rec = rec.reshape(len(rec), -1) if rec.size else rec.reshape(0, 8)
    boxes = record_boxes(rec)
    fr = rec[:, 0].astype(np.int64) - frame_offset
    return [candidate_mask(s, boxes[fr == f]) for f, s in enumerate(im_shapes)]


def masked_image(frame: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """rgb & (mask != 0): every byte of a pixel kept where the label is non-zero, 0 elsewhere; frame (rows, cols[, channels]) uint8"""
    keep = np.where(labels != 0, np.uint8(0xFF), np.uint8(0))
    return frame & (keep[..., None] if frame.ndim == 3 else keep)


def _quaternion(M):
    """Eigen's Quaternion(const Matrix3 &) in double, then normalize(): (x, y, z, w)"""
    q = [0.0, 0.0, 0.0, 0.0]
    tr = (M[0][0] + M[1][1]) + M[2][2]
    if tr > 0.0:
        t = math.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (M[2][1] - M[1][2]) * t
        q[1] = (M[0][2] - M[2][0]) * t
        q[2] = (M[1][0] - M[0][1]) * t
    else:
        i = 0
        if M[1][1] > M[0][0]:
            i = 1
        if M[2][2] > M[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((M[i][i] - M[j][j]) - M[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (M[k][j] - M[j][k]) * t
        q[j] = (M[j][i] + M[i][j]) * t
        q[k] = (M[k][i] + M[i][k]) * t
    nrm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [v / nrm for v in q]


def pose_frame(C):
    """(eigenvalues ascending, frame M as rows of a 3x3 list) of a symmetric 3x3 of Python floats: the Jacobi eigenpairs, columns 0
    and 1 the two smallest eigenvalues' vectors with their largest-magnitude component made positive, column 2 their cross product"""
    A = [list(r) for r in C]
    V = jacobi3(A)
    o = [0, 1, 2]
    for k in (1, 2):                       # stable insertion sort: ties keep index order
        j = k
        while j > 0 and A[o[j]][o[j]] < A[o[j - 1]][o[j - 1]]:
            o[j], o[j - 1] = o[j - 1], o[j]
            j -= 1
    M = [[0.0] * 3 for _ in range(3)]
    for col in (0, 1):
        v = [V[r][o[col]] for r in range(3)]
        big = 0
        for k in (1, 2):
            if abs(v[k]) > abs(v[big]):
                big = k
        if v[big] < 0.0:
            v = [-e for e in v]
        for r in range(3):
            M[r][col] = v[r]
    M[0][2] = M[1][0] * M[2][1] - M[2][0] * M[1][1]
    M[1][2] = M[2][0] * M[0][1] - M[0][0] * M[2][1]
    M[2][2] = M[0][0] * M[1][1] - M[1][0] * M[0][1]
    return [A[o[k]][o[k]] for k in range(3)], M


def part_poses(centres: np.ndarray, ncentres: np.ndarray, dense: np.ndarray):
    """messagePoses per record on what computeBoundingBoxes returns: centres (n, max_parts, 3) float32, ncentres (n,), dense (n,).
    Returns count (n,) int32, position (n, 3), orientation (n, 4) as (x, y, z, w) and eigenvalues (n, 3) ascending, float32;
    NaN where count is 0 (and orientation / eigenvalues NaN where the covariance is not finite)."""
    cen = np.asarray(centres, np.float32)
    n = len(cen)
    cen = cen.reshape(n, -1, 3)
    nc = np.asarray(ncentres, np.int64).reshape(n)
    dn = np.asarray(dense).reshape(n) != 0
    acc = np.zeros((9, n), np.float32)     # xx, xy, xz, yy, yz, zz, x, y, z: fp32 sums in point order, vectorised over records
    cnt = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for j in range(cen.shape[1]):
            x, y, z = cen[:, j, 0], cen[:, j, 1], cen[:, j, 2]
            use = (j < nc) & (dn | (np.isfinite(x) & np.isfinite(y) & np.isfinite(z)))
            for k, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
                acc[k] = np.where(use, acc[k] + v, acc[k])
            cnt += use
        fc = cnt.astype(np.float32)
        m = acc / fc
        c = np.stack([m[0] - m[6] * m[6], m[1] - m[6] * m[7], m[2] - m[6] * m[8], m[3] - m[7] * m[7], m[4] - m[7] * m[8],
                      m[5] - m[8] * m[8]]) / fc
    pos = np.full((n, 3), np.nan, np.float32)
    quat = np.full((n, 4), np.nan, np.float32)
    ev = np.full((n, 3), np.nan, np.float32)
    for i in range(n):
        if cnt[i] == 0:
            continue
        pos[i] = m[6:9, i]
        if not np.isfinite(c[:, i]).all():
            continue
        a = [float(v) for v in c[:, i]]
        lam, M = pose_frame([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])
        ev[i] = np.array(lam, np.float64).astype(np.float32)
        quat[i] = np.array(_quaternion(M), np.float64).astype(np.float32)
    return cnt, pos, quat, ev
