"""Numpy yardstick of pbd_top_k_cells / pbd_set_top_k / pbd_top_k (include/pbd.h states the rule): of each segment the
min(K, eligible) best eligible elements, a better than b when its value is larger or, the values being equal, its index smaller;
NaN and masked elements take no part; +0.0 and -0.0 tie.

A literal sort-based restatement.  Nothing here runs on the GPU; the device result must equal it byte for byte.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def eligible(values: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """the elements that take part: not NaN and, with a mask, a non-zero mask element"""
    ok = ~np.isnan(values)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


def top_k_cells_ref(values: np.ndarray, k: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """one segment (raveled in C order): the uint8 array of 0 / 255 in values' shape, 255 at the min(k, eligible) best eligible
    elements.  The comparisons are made in values' dtype."""
    v = np.asarray(values)
    if k < 0:
        raise ValueError("top_k_cells_ref: k >= 0")
    flat = v.ravel()
    idx = np.flatnonzero(eligible(flat, None if mask is None else np.asarray(mask).ravel()))
    # the total order: value descending, then index ascending.  A stable sort of the ascending indices by the negated value keeps
    # equal values -- the two zeros included, -(-0.0) == -(+0.0) -- in index order
    order = idx[np.argsort(-flat[idx], kind="stable")]
    dst = np.zeros(flat.size, np.uint8)
    dst[order[:k]] = 255
    return dst.reshape(v.shape)


def top_k_segments_ref(segments: Sequence[np.ndarray], k: int, masks: Optional[Sequence[Optional[np.ndarray]]] = None):
    """top_k_cells_ref of every segment"""
    return [top_k_cells_ref(s, k, None if masks is None else masks[i]) for i, s in enumerate(segments)]


def top_k_records_ref(records: np.ndarray, k: int) -> np.ndarray:
    """the records (n, stride) int32 kept by pbd_top_k, in input order: per value of word 0 (the frame) the k best by the float
    score in word 5, ties to the earlier record, a NaN score never"""
    rec = np.asarray(records, np.int32)
    if not len(rec):
        return rec
    rec = rec.reshape(len(rec), -1)
    score = np.ascontiguousarray(rec[:, 5]).view(np.float32)
    keep = np.zeros(len(rec), bool)
    for f in np.unique(rec[:, 0]):
        idx = np.flatnonzero(rec[:, 0] == f)
        keep[idx[top_k_cells_ref(score[idx], k) != 0]] = True
    return rec[keep]


def canonical_order(records: np.ndarray) -> np.ndarray:
    """the records sorted by (frame, level, component, y, x) -- words 0, 2, 1, 4, 3 -- the order the find lists them in"""
    rec = np.asarray(records, np.int32)
    if not len(rec):
        return rec
    rec = rec.reshape(len(rec), -1)
    return rec[np.lexsort((rec[:, 3], rec[:, 4], rec[:, 1], rec[:, 2], rec[:, 0]))]
