"""Numpy yardstick of pbd_grid_nms / pbd_set_root_nms (include/pbd.h states the contract):
nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129), the block NMS of Neubeck and Van Gool, with the project's
decisions -- a block without an eligible element has no maximum, an empty neighbourhood beats nothing, NaN is never eligible.

Nothing here runs on the GPU; the device result must equal `grid_nms_ref` byte for byte.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def eligible(src: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """the elements that take part: not NaN and, with a mask, a non-zero mask element"""
    ok = ~np.isnan(src)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


def grid_nms_ref(src: np.ndarray, sz: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """the uint8 plane of 0 / 255: 255 at a block's candidate (its largest eligible element, the first in raster order among equal
    ones) when it is strictly greater than every eligible element of its window of 2 sz + 1 that lies outside its own block.  The
    comparisons are made in src's dtype."""
    src = np.asarray(src)
    if src.ndim != 2 or not 0 <= sz <= 32767:
        raise ValueError("grid_nms_ref: a 2-D plane and 0 <= sz <= 32767")
    M, N = src.shape
    ok = eligible(src, mask)
    dst = np.zeros((M, N), np.uint8)
    bs = sz + 1
    for m in range(0, M, bs):
        for n in range(0, N, bs):
            blk, bok = src[m:m + bs, n:n + bs], ok[m:m + bs, n:n + bs]
            if not bok.any():
                continue                                   # an empty block has no maximum
            vals = blk[bok]
            vc = vals.max()
            first = np.flatnonzero(bok.ravel() & (blk.ravel() == vc))[0]     # == ties -0.0 with +0.0
            cy, cx = m + first // blk.shape[1], n + first % blk.shape[1]
            y0, x0 = max(cy - sz, 0), max(cx - sz, 0)
            win, wok = src[y0:cy + sz + 1, x0:cx + sz + 1], ok[y0:cy + sz + 1, x0:cx + sz + 1].copy()
            wok[m - y0:m - y0 + bs, n - x0:n - x0 + bs] = False            # minus the candidate's own block
            if wok.any() and not vc > win[wok].max():
                continue
            dst[cy, cx] = 255
    return dst


def filter_records(records: np.ndarray, kept) -> np.ndarray:
    """the records (n, stride) int32 whose root cell is a maximum, in input order: kept(frame, level, component) is the uint8 plane
    grid_nms_ref returned for that rootv plane; the root is words 3 (x) and 4 (y) of a record"""
    rec = np.asarray(records, np.int32)
    rec = rec.reshape(len(rec), -1)
    keep = [bool(kept(int(r[0]), int(r[2]), int(r[1]))[int(r[4]), int(r[3])]) for r in rec]
    return rec[np.array(keep, bool)] if len(rec) else rec
