"""The padded pyramid, restated in numpy: the yardstick of pbd_set_padding (include/pbd.h).

The Matlab detector pads every feature level by a border of cells that hold 0 on every channel but the last and 1 on the last
(the "boundary occlusion feature", featpyramid.m:36-45), places roots and parts on the larger map and takes the pad off again in
the box arithmetic (detect.m:266-270).  Three statements make the rule:

  * ``pad_features``: what a padded plane holds;
  * the part rectangle is ``examples.part_rects(x - padx, y - pady, ...)`` for a plane cell (x, y);
  * ``detect_ref``: the detector on padded planes, every step but these two the oracle's own.

Nothing here runs on the GPU.
"""
from __future__ import annotations

from typing import List

import numpy as np

from . import examples

MAX_PAD = 31   # the largest filter side (pbd_set_padding's range)


def check_pad(padx: int, pady: int) -> None:
    if not (0 <= int(padx) <= MAX_PAD and 0 <= int(pady) <= MAX_PAD):
        raise ValueError(f"padding ({padx}, {pady}) outside 0..{MAX_PAD}")


def pad_features(feat: np.ndarray, padx: int, pady: int, flen: int = 32) -> np.ndarray:
    """(H, W*flen) -> (H + 2 pady, (W + 2 padx) * flen): the interior copied, pad cells +0 on channels 0 .. flen-2 and 1 on
    channel flen-1.  A level with H == 0 or W == 0 stays empty (an empty level is never padded)."""
    check_pad(padx, pady)
    feat = np.asarray(feat)
    H, W = feat.shape[0], feat.shape[1] // flen
    if H == 0 or W == 0:
        return feat.copy()
    out = np.zeros((H + 2 * pady, W + 2 * padx, flen), feat.dtype)
    out[:, :, flen - 1] = 1
    out[pady:pady + H, padx:padx + W] = feat.reshape(H, W, flen)
    return out.reshape(H + 2 * pady, (W + 2 * padx) * flen)


def detect_ref(model, im: np.ndarray, padx: int = 0, pady: int = 0, dtype=np.float32, walk: str = "reference",
               rect_pad=None) -> List[dict]:
    """the detector on padded planes: oracle.features_pyramid -> pad_features -> oracle.responses -> oracle.dp_min (walk
    "argmax": examples.raw_maps) -> raster find with rootv > T(float32(thresh)) -> examples.walk -> padded rectangles.  Records
    (dicts as oracle.detect returns them) come in (level, component, y, x) order; root_x / root_y are plane coordinates (the
    image cell is root_x - padx).  ``model`` is a Model or its flattened form.  rect_pad: the pad the rectangles take off, when
    it is not (padx, pady) -- the changed rule of the tests."""
    from oracle import oracle
    flat = model.flatten() if hasattr(model, "flatten") else model
    T = np.dtype(dtype).type
    rx, ry = (padx, pady) if rect_pad is None else rect_pad
    thresh = T(np.float32(flat.thresh))
    feats, scales = oracle.features_pyramid(flat, im, dtype)
    out = []
    for lvl, f in enumerate(feats):
        feat = pad_features(f, padx, pady, flat.flen)
        if feat.size == 0:
            continue
        resp = oracle.responses(flat, feat)
        for c in range(flat.ncomponents):
            fn = examples.raw_maps if walk == "argmax" else oracle.dp_min
            Ix, Iy, Ik, rootv, rooti = fn(flat, c, resp)
            p0 = int(flat.part_offset[c])
            ys, xs = np.nonzero(rootv > thresh)          # raster order
            for y, x in zip(ys.tolist(), xs.tolist()):
                parts = []
                for p, (px, py, m) in enumerate(examples.walk(flat, c, x, y, Ix, Iy, Ik, rooti, argmax=walk == "argmax")):
                    k = int(flat.filter_ksize[flat.filterid[int(flat.mix_offset[p0 + p]) + m]])
                    x1, y1, x2, y2 = examples.part_rects(px, py, k, scales[lvl], dtype, pad=(rx, ry))
                    parts.append((int(x1), int(y1), int(x2 - x1), int(y2 - y1)))
                out.append({"component": c, "level": lvl, "root_x": x, "root_y": y, "score": float(np.float32(rootv[y, x])),
                            "parts": np.asarray(parts, np.int32)})
    return out
