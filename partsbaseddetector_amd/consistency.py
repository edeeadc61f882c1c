"""Numpy yardstick of pbd_depth_consistency (include/pbd.h states the contract):
SearchSpacePruning<T>::filterCandidatesByDepth(parts, candidates, depth, zfactor) (src/SearchSpacePruning.cpp:73-95) with the
project's decisions -- part boxes clipped to the depth image, NaN samples read as 0, a one-part component keeps its records.

Nothing here runs on the GPU; the device filter must equal `filter_records` record for record.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np


def samples(depth: np.ndarray, box, dtype) -> np.ndarray:
    """the samples of box (x, y, w, h) & Rect(0, 0, dcols, drows) as T (`dtype`): 8U / 16U exactly, 64F rounded to nearest when
    T is float; NaN reads as 0"""
    x, y, w, h = (int(v) for v in box)
    drows, dcols = depth.shape[:2]
    x1, y1 = max(x, 0), max(y, 0)
    x2, y2 = min(x + w, dcols), min(y + h, drows)
    if x2 - x1 <= 0 or y2 - y1 <= 0:
        return np.zeros(0, dtype)
    with np.errstate(over="ignore"):                  # a double beyond FLT_MAX rounds to Inf
        s = np.asarray(depth[y1:y2, x1:x2]).astype(dtype).ravel()
    s[np.isnan(s)] = 0
    return s


def median(s: np.ndarray) -> Optional[float]:
    """the element at index M / 2 of the ascending order (std::nth_element's middle: the upper median for even M); None when empty"""
    M = s.size
    if M == 0:
        return None
    return np.partition(s, M // 2)[M // 2]


def anchor_norms(flat) -> np.ndarray:
    """per global part: std::sqrt((double)ax*ax + (double)ay*ay) of its mixture-0 anchor (part.anchor(0)); 0 for a root"""
    out = np.zeros(len(flat.parentid), np.float64)
    for c in range(flat.ncomponents):
        for gp in range(int(flat.part_offset[c]) + 1, int(flat.part_offset[c + 1])):
            ax, ay = (float(v) for v in flat.anchors[int(flat.defid[int(flat.mix_offset[gp])])])
            out[gp] = math.sqrt(ax * ax + ay * ay)
    return out


def keep_record(flat, rec: np.ndarray, depth: np.ndarray, zfactor: float, dtype, norms: Optional[np.ndarray] = None) -> bool:
    """the reference's decision for one record (int32 words: header, then x, y, w, h per part)"""
    dtype = np.dtype(dtype).type
    norms = anchor_norms(flat) if norms is None else norms
    c, npart = int(rec[1]), int(rec[6])
    p0 = int(flat.part_offset[c])
    if npart == 1:                       # project decision: a one-part component keeps its records
        return True
    med = [median(samples(depth, rec[8 + 4 * j:12 + 4 * j], dtype)) for j in range(npart)]
    z = float(np.float32(zfactor))
    for p in range(1, npart):
        q = int(flat.parentid[p0 + p])
        mc, mq = med[p], med[q]
        if mc is None or mq is None or not (mc > 0 and mq > 0):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = abs(dtype(mc) - dtype(mq))                  # in T
        if float(d) > norms[p0 + p] * z:                    # a NaN difference compares false
            return False
    return True


def filter_records(flat, records: np.ndarray, depths: Sequence[np.ndarray], zfactor: float = 0.03, dtype=np.float32,
                   frame_offset: int = 0) -> np.ndarray:
    """the kept records (n, stride) int32, in input order, unchanged; depths[f] is the depth image of frame index f
    (record frame field - frame_offset)"""
    rec = np.asarray(records, np.int32)
    rec = rec.reshape(len(rec), -1) if rec.size else rec.reshape(0, max(rec.shape[-1] if rec.ndim == 2 else 8, 8))
    norms = anchor_norms(flat)
    keep = [keep_record(flat, r, depths[int(r[0]) - frame_offset], zfactor, dtype, norms) for r in rec]
    return rec[np.array(keep, bool)] if len(rec) else rec
