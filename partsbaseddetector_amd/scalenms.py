"""Numpy yardstick of pbd_set_scale_nms / pbd_scale_nms (include/pbd.h states the rule): an eligible root is kept iff no eligible
neighbour is better.  Two roots of a frame are neighbours when their levels are at most dl apart and the doubled centre of one's
root rectangle lies inside the other's half-open rectangle; a is better than b when its score is larger or, the scores being
equal, it comes earlier in the find order (level, component, y, x).  All geometry is integer.

Two formulations that must agree: `keep_records`, all pairs over a record list (the rule as written), and `keep_planes`, per root
cell over windows of the neighbouring (level, component) planes (the kernel's shape, its window bound included).

Nothing here runs on the GPU; the device result must equal it record for record.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np


def _rows(rec: np.ndarray) -> np.ndarray:
    """(n, stride) of a record array; an empty one keeps the stride it has"""
    if rec.size:
        return rec.reshape(len(rec), -1)
    return rec.reshape(0, rec.shape[-1] if rec.ndim == 2 and rec.shape[-1] else 12)


def covers(a, b) -> bool:
    """covers(a, b) for rectangles (x, y, w, h): b's centre, doubled, inside a's half-open rectangle"""
    xa, ya, wa, ha = (int(v) for v in a)
    xb, yb, wb, hb = (int(v) for v in b)
    cx, cy = 2 * xb + wb, 2 * yb + hb
    return wa > 0 and ha > 0 and 2 * xa <= cx < 2 * (xa + wa) and 2 * ya <= cy < 2 * (ya + ha)


def neighbours(ra, la, rb, lb, dl: int) -> bool:
    """two different roots of one frame with rectangles ra, rb on levels la, lb"""
    return abs(int(la) - int(lb)) <= dl and (covers(ra, rb) or covers(rb, ra))


def better(sa, ia, sb, ib) -> bool:
    """a (score sa, position ia in the find order) is better than b; the scores are compared in their own dtype"""
    return bool(sa > sb) or (bool(sa == sb) and ia < ib)


def keep_records(records: np.ndarray, dl: int, scores: Optional[np.ndarray] = None, frame_offset: int = 0,
                 nframes: Optional[int] = None, max_parts: Optional[int] = None) -> np.ndarray:
    """per record (n, stride) int32, in the find order: kept?  All pairs.  `scores` (default: the records' float scores, word 5)
    are the values compared, e.g. rootv in float64.  A record with a NaN score, a frame index (word 0 - frame_offset) outside
    0 .. nframes - 1 (where nframes is given) or nparts outside 1..max parts (default: what the stride holds) is dropped and is
    nobody's neighbour."""
    rec = _rows(np.asarray(records, np.int32))
    n = len(rec)
    if not 0 <= int(dl) <= 255:
        raise ValueError("scale NMS: dl in 0..255")
    s = np.ascontiguousarray(rec[:, 5]).view(np.float32) if scores is None else np.asarray(scores)
    mp = (rec.shape[1] - 8) // 4 if max_parts is None else max_parts
    ok = ~np.isnan(s) & (rec[:, 6] >= 1) & (rec[:, 6] <= mp) & (rec[:, 0].astype(np.int64) - frame_offset >= 0)
    if nframes is not None:
        ok &= rec[:, 0].astype(np.int64) - frame_offset < nframes
    keep = ok.copy()
    f, lv = rec[:, 0], rec[:, 2].astype(np.int64)
    x, y, w, h = (rec[:, 8 + k].astype(np.int64) for k in range(4))
    cx, cy, idx = 2 * x + w, 2 * y + h, np.arange(n)
    for i in np.flatnonzero(ok):
        # record i against every record j at once: the rule's clauses in its order
        near = ok & (idx != i) & (f == f[i]) & (np.abs(lv - lv[i]) <= dl)
        i_covers_j = (w[i] > 0) & (h[i] > 0) & (2 * x[i] <= cx) & (cx < 2 * (x[i] + w[i])) & (2 * y[i] <= cy) & (cy < 2 * (y[i] + h[i]))
        j_covers_i = (w > 0) & (h > 0) & (2 * x <= cx[i]) & (cx[i] < 2 * (x + w)) & (2 * y <= cy[i]) & (cy[i] < 2 * (y + h))
        j_better = (s > s[i]) | ((s == s[i]) & (idx < i))
        if np.any(near & (i_covers_j | j_covers_i) & j_better):
            keep[i] = False
    return keep


def filter_records(records: np.ndarray, dl: int, scores: Optional[np.ndarray] = None, frame_offset: int = 0,
                   nframes: Optional[int] = None) -> np.ndarray:
    """the kept records (n, stride) int32, in input order, unchanged"""
    rec = _rows(np.asarray(records, np.int32))
    return rec[keep_records(rec, dl, scores, frame_offset, nframes)]


# ---- the plane form ----------------------------------------------------------------------------------------------------------
@dataclass
class Level:
    """one pyramid level of a frame: its scale (cast to the planes' dtype), the pad of pbd_set_padding, and per component the
    planes rootv (rows, cols), rooti (rows, cols) and the optional mask bytes (root NMS and depth pruning, already combined)"""
    scale: float
    rootv: List[np.ndarray]
    rooti: List[np.ndarray]
    padx: int = 0
    pady: int = 0
    mask: Optional[List[Optional[np.ndarray]]] = None


def round_mul(a, s, dtype):
    """cv::Point_<int> * T: the product in T, rounded half to even"""
    return int(np.rint(dtype(a) * dtype(s)))


def part_rect(x: int, y: int, ks: int, scale, dtype, padx: int = 0, pady: int = 0):
    """(x, y, w, h) of the root at plane cell (x, y) with filter side ks, as the walk writes it (src/DynamicProgram.cpp:238-241)"""
    dtype = np.dtype(dtype).type
    x1, y1 = round_mul(x - padx - 1, scale, dtype), round_mul(y - pady - 1, scale, dtype)
    x2, y2 = x1 + round_mul(ks, scale, dtype) - 1, y1 + round_mul(ks, scale, dtype) - 1
    return min(x1, x2), min(y1, y2), abs(x2 - x1), abs(y2 - y1)


def window(xa: int, wa: int, wmax: int, s: float, pad: int, n: int):
    """the cells [c0, c1) of one axis of a neighbour plane (scale s, pad, n cells) that can hold a neighbour of a root spanning
    [xa, xa + wa] on that axis when no rectangle of the plane is wider than wmax: a cell's X = round((c - pad - 1) * s) must
    satisfy xa - wmax <= X <= xa + wa + 1 (include/pbd.h's two covers, either way); one unit for the rounding and one cell for
    the division are added on either side"""
    if not s > 0:
        return 0, n
    lo = math.floor((xa - wmax - 1) / s) + pad
    hi = math.ceil((xa + wa + 2) / s) + pad + 2
    c0 = 0 if lo <= 0 else min(lo, n)
    c1 = n if hi >= n - 1 else (hi + 1 if hi >= 0 else 0)
    return c0, c1


def keep_planes(levels: Sequence[Level], root_ksize: Sequence[Sequence[int]], thresh, dl: int, use_window: bool = True):
    """one frame: levels[l] as above, root_ksize[c][m] the filter side of root type m of component c.  Returns keep[l][c], uint8
    planes of 0 / 255.  Eligible: rootv > thresh in the planes' dtype, and the mask byte where given.  Each eligible cell looks
    through the windows of the planes within dl levels (use_window False: through every cell of them)."""
    if not 0 <= int(dl) <= 255:
        raise ValueError("scale NMS: dl in 0..255")
    nl, nc = len(levels), len(root_ksize)
    keep = [[np.zeros(np.asarray(L.rootv[c]).shape, np.uint8) for c in range(nc)] for L in levels]
    if not nl:
        return keep
    dtype = np.asarray(levels[0].rootv[0]).dtype.type
    thr = dtype(thresh)

    def elig(l, c):
        v = np.asarray(levels[l].rootv[c])
        e = v > thr
        m = levels[l].mask[c] if levels[l].mask is not None else None
        return e & (np.asarray(m) != 0) if m is not None else e

    E = [[elig(l, c) for c in range(nc)] for l in range(nl)]
    rects = {}

    def rect(l, c, y, x):
        key = (l, c, y, x)
        if key not in rects:
            L = levels[l]
            rects[key] = part_rect(x, y, root_ksize[c][int(L.rooti[c][y, x])], L.scale, dtype, L.padx, L.pady)
        return rects[key]

    for l in range(nl):
        for c in range(nc):
            for y, x in zip(*np.nonzero(E[l][c])):
                ra, sa, ia = rect(l, c, y, x), levels[l].rootv[c][y, x], (l, c, y, x)
                beaten = False
                for l2 in range(max(l - dl, 0), min(l + dl, nl - 1) + 1):
                    L2 = levels[l2]
                    for c2 in range(nc):
                        rows, cols = np.asarray(L2.rootv[c2]).shape
                        if rows * cols == 0:
                            continue
                        if use_window:
                            wmax = round_mul(max(root_ksize[c2]), L2.scale, dtype) + 1
                            x0, x1 = window(ra[0], ra[2], wmax, float(dtype(L2.scale)), L2.padx, cols)
                            y0, y1 = window(ra[1], ra[3], wmax, float(dtype(L2.scale)), L2.pady, rows)
                        else:
                            x0, x1, y0, y1 = 0, cols, 0, rows
                        for y2 in range(y0, y1):
                            for x2 in range(x0, x1):
                                ib = (l2, c2, y2, x2)
                                if ib == ia or not E[l2][c2][y2, x2] or not better(L2.rootv[c2][y2, x2], ib, sa, ia):
                                    continue
                                rb = rect(l2, c2, y2, x2)
                                if covers(ra, rb) or covers(rb, ra):
                                    beaten = True
                                    break
                            if beaten:
                                break
                        if beaten:
                            break
                    if beaten:
                        break
                if not beaten:
                    keep[l][c][y, x] = 255
    return keep


def plane_records(levels: Sequence[Level], root_ksize: Sequence[Sequence[int]], planes, frame: int = 0, stride: int = 12):
    """the records (n, stride) int32 of the non-zero cells of planes[l][c] in the find order -- header, nparts 1 and the root
    rectangle -- and their scores in the planes' dtype"""
    dtype = np.asarray(levels[0].rootv[0]).dtype.type if len(levels) else np.float32
    rows, scores = [], []
    for l, L in enumerate(levels):
        for c in range(len(root_ksize)):
            for y, x in zip(*np.nonzero(planes[l][c])):
                r = np.zeros(stride, np.int32)
                m = int(L.rooti[c][y, x])
                r[:5] = (frame, c, l, x, y)
                r[5] = np.array([L.rootv[c][y, x]]).astype(np.float32).view(np.int32)[0]
                r[6], r[7] = 1, m
                r[8:12] = part_rect(x, y, root_ksize[c][m], L.scale, dtype, L.padx, L.pady)
                rows.append(r)
                scores.append(L.rootv[c][y, x])
    return np.array(rows, np.int32).reshape(len(rows), stride), np.array(scores, dtype)
