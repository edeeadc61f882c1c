"""Numpy yardstick of pbd_set_depth_prune / pbd_depth_prune (include/pbd.h states the contract): a root box w pixels wide of an
object `width` wide must stand at depth Z = fx * width / w -- the intent of SearchSpacePruning::filterResponseByDepth
(src/SearchSpacePruning.cpp:47-70), with the project's arithmetic: nine samples of the clipped root rectangle, holes skipped, kept
when any valid sample lies within tol * Z of Z or none is valid.

Nothing here runs on the GPU; the device must equal `plausible` decision for decision, for every depth dtype and both real types.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def _rows(rec: np.ndarray) -> np.ndarray:
    """(n, stride) of a record array; an empty one keeps the stride it has"""
    if rec.size:
        return rec.reshape(len(rec), -1)
    return rec.reshape(0, rec.shape[-1] if rec.ndim == 2 and rec.shape[-1] else 12)


def sample_points(rect, rows: int, cols: int) -> List[Tuple[int, int]]:
    """the nine (py, px) sample points of rect = (x, y, w, h) clipped to a rows x cols image, row by row; [] when the clipped
    rectangle is empty"""
    x, y, w, h = (int(v) for v in rect)
    x1, y1 = max(x, 0), max(y, 0)
    x2, y2 = min(x + w, int(cols)), min(y + h, int(rows))
    if x2 - x1 <= 0 or y2 - y1 <= 0:
        return []
    return [(y1 + ((2 * j + 1) * (y2 - y1)) // 6, x1 + ((2 * i + 1) * (x2 - x1)) // 6) for j in range(3) for i in range(3)]


def plausible(rect, depth: np.ndarray, fx: float, width: float, tol: float) -> bool:
    """the rule for one root rectangle (x, y, w, h) and its frame's depth image (2-D: uint8, uint16, float32 or float64)"""
    w = int(rect[2])
    if w <= 0:
        return True
    pts = sample_points(rect, depth.shape[0], depth.shape[1])
    if not pts:
        return True
    fx, width, tol = (np.float64(np.float32(v)) for v in (fx, width, tol))
    Z = (fx * width) / np.float64(w)
    band = tol * Z
    valid = False
    for py, px in pts:
        d = np.float64(depth[py, px])
        if not (d > 0 and d < np.inf):        # NaN, zeros, negatives and Inf are holes
            continue
        valid = True
        if abs(d - Z) <= band:
            return True
    return not valid                          # unknown depth never prunes


def keep_mask(records: np.ndarray, depths: Sequence[np.ndarray], fx: float, width: float, tol: float, frame_offset: int = 0,
              max_parts: Optional[int] = None) -> np.ndarray:
    """per record (n, stride) int32: kept?  A record whose frame index (frame field - frame_offset) is outside depths, or whose
    nparts is outside 1..max parts (default: what the stride holds), is dropped"""
    rec = np.asarray(records, np.int32)
    rec = _rows(rec)
    mp = (rec.shape[1] - 8) // 4 if max_parts is None else max_parts
    keep = np.zeros(len(rec), bool)
    for k, r in enumerate(rec):
        f = int(r[0]) - frame_offset
        if f < 0 or f >= len(depths) or not 1 <= int(r[6]) <= mp:
            continue
        keep[k] = plausible(r[8:12], depths[f], fx, width, tol)
    return keep


def filter_records(records: np.ndarray, depths: Sequence[np.ndarray], fx: float, width: float, tol: float,
                   frame_offset: int = 0) -> np.ndarray:
    """the kept records (n, stride) int32, in input order, unchanged; depths[f] is the depth image of frame index f"""
    rec = np.asarray(records, np.int32)
    rec = _rows(rec)
    return rec[keep_mask(rec, depths, fx, width, tol, frame_offset)]


def eligible_planes(records: np.ndarray, depths: Sequence[np.ndarray], fx: float, width: float, tol: float, shapes) -> dict:
    """the uint8 planes of plausible cells above the threshold, for the root-NMS yardstick (gridnms.grid_nms_ref's mask): `records`
    are those of an unpruned, unsuppressed run -- one per root cell above the threshold -- and shapes[(frame, level)] = (rows, cols)
    of that level's root planes.  Returns {(frame, level, component): plane}; a key appears for every record's plane."""
    rec = np.asarray(records, np.int32)
    rec = _rows(rec)
    out: dict = {}
    for r, k in zip(rec, keep_mask(rec, depths, fx, width, tol)):
        key = (int(r[0]), int(r[2]), int(r[1]))
        if key not in out:
            out[key] = np.zeros(shapes[(key[0], key[1])], np.uint8)
        if k:
            out[key][int(r[4]), int(r[3])] = 1
    return out
