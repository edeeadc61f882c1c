"""Warped positives, restated in numpy: the yardstick of pbd_warp_positives* (include/pbd.h).

poswarp of the reference's Matlab training code (matlab/learning/train.m:131-162 with warppos.m, subarray.m and qp_poswrite):
every annotated box is padded by one cell, cropped with edge replication, resized to (k + 2) * sbin pixels, and its HOG written
as the example [bias = 1 | filter block = feat] in pbd_examples' format.

Nothing here runs on the GPU.  The resize and the HOG are the CPU oracle's (cv::resize INTER_LINEAR and HOGFeatures<T>::features
as the detector restates them): Matlab's imresize and its double-precision features.cc are not reproduced, on purpose -- the
example holds what the detector itself computes on the patch.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence, Tuple

import numpy as np

from . import examples as ex


def matlab_round(v: float) -> int:
    """Matlab's round: halves away from zero"""
    r = math.trunc(v)
    return r + (1 if v > 0 else -1) if abs(v - r) >= 0.5 else r   # v - r is exact


def window(box, k: int, sbin: int) -> Tuple[int, int, int, int]:
    """(x0, y0, width, height) of the padded window of box = (x1, y1, x2, y2), 0-based inclusive: its first column and row
    (0-based, may be negative) and its size.  warppos.m:21-26 in Matlab's 1-based coordinates, then shifted by one."""
    x1, y1, x2, y2 = (int(v) for v in box)
    width, height = x2 - x1 + 1, y2 - y1 + 1
    padx = float(sbin) * width / (float(k) * sbin)
    pady = float(sbin) * height / (float(k) * sbin)
    X1, X2 = matlab_round((x1 + 1) - padx), matlab_round((x2 + 1) + padx)
    Y1, Y2 = matlab_round((y1 + 1) - pady), matlab_round((y2 + 1) + pady)
    return X1 - 1, Y1 - 1, X2 - X1 + 1, Y2 - Y1 + 1


def crop(im: np.ndarray, box, k: int, sbin: int) -> np.ndarray:
    """subarray(im, Y1, Y2, X1, X2, 1): the window's pixels, those outside the frame replicated from its edge"""
    im = im if im.ndim == 3 else im[:, :, None]
    x0, y0, w, h = window(box, k, sbin)
    ys = np.clip(np.arange(y0, y0 + h), 0, im.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, im.shape[1] - 1)
    return np.ascontiguousarray(im[ys][:, xs])


def patch(im: np.ndarray, box, k: int, sbin: int) -> np.ndarray:
    """the P x P patch of a box, P = (k + 2) * sbin: the clamped gather, then the oracle's cv::resize INTER_LINEAR"""
    from oracle import oracle
    win = crop(im, box, k, sbin)
    P = (k + 2) * sbin
    if win.dtype == np.uint8:
        return oracle.resize_linear_u8(win, P, P)
    r, c, cn = win.shape
    dst = np.empty((P, P, cn), win.dtype)
    oracle.lib().pbdo_resize_linear(C.c_void_p(win.ctypes.data), oracle.DEPTH_CODE[win.dtype], r, c, cn, C.c_size_t(c * cn),
                                    C.c_void_p(dst.ctypes.data), P, P, C.c_size_t(P * cn))
    return dst


def keeps(box, k: int, sbin: int, skip_small: bool = True) -> bool:
    """train.m:135-143: a box smaller than the filter's pixels is skipped (minsize = prod(model.maxsize * model.sbin))"""
    x1, y1, x2, y2 = (int(v) for v in box)
    return not (skip_small and float(x2 - x1 + 1) * float(y2 - y1 + 1) < (float(k) * sbin) ** 2)


def warp_examples(flat, frames: Sequence[np.ndarray], boxes, filter: int = 0, bias: int = 0, skip_small: bool = True,
                  dtype=np.float32):
    """(hdr (n, hdr_words) int32, values (n, values) T, kept (n,) int32) of boxes (n, 5) = frame, x1, y1, x2, y2: what
    pbd_warp_positives returns into zero-filled arrays"""
    from oracle import oracle
    boxes = np.asarray(boxes, np.int64).reshape(-1, 5)
    hdr_words, vstride = ex.strides(flat)
    _, fbase, _ = ex.vector_offsets(flat)
    k, sbin = int(flat.filter_ksize[filter]), int(flat.sbin)
    n = len(boxes)
    H = np.zeros((n, hdr_words), np.int32)
    V = np.zeros((n, vstride), dtype)
    kept = np.zeros(n, np.int32)
    for i, (f, *box) in enumerate(boxes):
        H[i, 0] = i
        if not keeps(box, k, sbin, skip_small):
            H[i, 2] = -1
            continue
        kept[i] = 1
        feat = oracle.hog_features(patch(frames[int(f)], box, k, sbin), sbin, flat.norient, flat.flen, dtype)
        assert feat.shape == (k, k * flat.flen), feat.shape
        blocks, vals = [], []
        if bias >= 0:
            blocks.append((bias, 1))
            vals.append(np.ones(1, dtype))
        blocks.append((fbase + int(flat.filter_offset[filter]), k * k * flat.flen))
        vals.append(feat.ravel())
        v = np.concatenate(vals)
        H[i, 2:4] = (len(blocks), len(v))
        H[i, 4:4 + 2 * len(blocks)] = np.asarray(blocks, np.int32).ravel()
        V[i, :len(v)] = v
    return H, V, kept
