"""The fine octave, restated in numpy: the yardstick of pbd_set_fine_octave (include/pbd.h).

The detector's smallest scale is the frame itself at the model's bin size, so an object smaller than the model's template cannot
be found.  Felzenszwalb's featpyramid computes the first ``interval`` levels a second time at bin size ``sbin / 2`` on the same
resampled images: an octave of levels at twice the feature resolution.  Three statements make the rule:

  * ``fine_features``: fine level i is the HOG of reference level i's IMAGE at bin size sbin // 2, its scale is scale[i] / 2;
  * ``features_pyramid``: the fine levels come first, the reference's levels follow unchanged, nfine = min(interval, nlevels) up;
  * ``detect_ref``: the detector over that level list, every other step that of padding.detect_ref.

Nothing here runs on the GPU.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import examples
from .padding import pad_features

MAX_LEVELS = 128   # PBD_MAX_LEVELS


def fine_sbin(sbin: int) -> int:
    """the bin size of the fine levels; an odd sbin or one below 4 has none (pbd_set_fine_octave refuses it)"""
    sbin = int(sbin)
    if sbin < 4 or sbin % 2:
        raise ValueError(f"a fine octave at bin size {sbin}: sbin / 2 must be an integer >= 2")
    return sbin // 2


def nfine(interval: int, nlevels: int) -> int:
    return min(int(interval), int(nlevels))


def plan(rows: int, cols: int, sbin: int, interval: int):
    """(img_rows, img_cols, feat_rows, feat_cols, scales, nfine) of the pyramid with the octave on: what pbd_pyramid_plan
    reports (without padding)"""
    from oracle import oracle
    fs = fine_sbin(sbin)
    lr, lc, sc = oracle.pyramid_plan(rows, cols, sbin, interval)
    nf = nfine(interval, len(lr))
    if len(lr) + nf > MAX_LEVELS:
        raise ValueError(f"{len(lr)} levels + {nf} of the fine octave exceed {MAX_LEVELS}")
    ir = np.concatenate([lr[:nf], lr]).astype(np.int32)
    ic = np.concatenate([lc[:nf], lc]).astype(np.int32)
    dims = [oracle.hog_dims(int(r), int(c), fs) for r, c in zip(lr[:nf], lc[:nf])] + \
           [oracle.hog_dims(int(r), int(c), sbin) for r, c in zip(lr, lc)]
    scales = np.concatenate([sc[:nf] / np.float32(2), sc]).astype(np.float32)
    return ir, ic, np.asarray([d[0] for d in dims], np.int32), np.asarray([d[1] for d in dims], np.int32), scales, nf


def fine_features(flat, im: np.ndarray, dtype=np.float32, scale_div=2, image_shift: int = 0, sbin=None) -> Tuple[List[np.ndarray], np.ndarray]:
    """the fine levels' feature maps (H, W*flen) and scales.  No image is resampled anew: fine level i reads the level image of
    reference level i.  scale_div, image_shift, sbin: the changed rules of the tests (the scale not halved, the HOG taken from
    level i + image_shift's image, another bin size)."""
    from oracle import oracle
    fs = fine_sbin(flat.sbin) if sbin is None else int(sbin)
    imgs, sc = oracle.pyramid_images(im, flat.sbin, flat.interval)
    nf = nfine(flat.interval, len(imgs))
    feats = [oracle.hog_features(imgs[min(i + image_shift, len(imgs) - 1)], fs, flat.norient, flat.flen, dtype=dtype) for i in range(nf)]
    scales = (np.asarray(sc[:nf], np.float32) / np.float32(scale_div)).astype(np.float32)
    return feats, scales


def features_pyramid(flat, im: np.ndarray, dtype=np.float32, fine: bool = True, **changed) -> Tuple[List[np.ndarray], np.ndarray]:
    """fine levels + oracle.features_pyramid: the level list of a handle with the octave on (fine False: the oracle's own)"""
    from oracle import oracle
    feats, scales = oracle.features_pyramid(flat, im, dtype)
    if not fine:
        return feats, scales
    ff, fs = fine_features(flat, im, dtype, **changed)
    if len(ff) + len(feats) > MAX_LEVELS:
        raise ValueError(f"{len(feats)} levels + {len(ff)} of the fine octave exceed {MAX_LEVELS}")
    return ff + list(feats), np.concatenate([fs, scales]).astype(np.float32)


def detect_ref(model, im: np.ndarray, fine: bool = True, padx: int = 0, pady: int = 0, dtype=np.float32, walk: str = "reference",
               **changed) -> List[dict]:
    """the detector over the level list of ``features_pyramid``: pad_features -> oracle.responses -> oracle.dp_min (walk
    "argmax": examples.raw_maps) -> raster find with rootv > T(float32(thresh)) -> examples.walk -> examples.part_rects with the
    level's scale.  Records (dicts as oracle.detect returns them) come in (level, component, y, x) order; ``level`` indexes the
    longer list.  fine False: padding.detect_ref record for record.  ``model`` is a Model or its flattened form."""
    from oracle import oracle
    flat = model.flatten() if hasattr(model, "flatten") else model
    T = np.dtype(dtype).type
    thresh = T(np.float32(flat.thresh))
    feats, scales = features_pyramid(flat, im, dtype, fine, **changed)
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
                    x1, y1, x2, y2 = examples.part_rects(px, py, k, scales[lvl], dtype, pad=(padx, pady))
                    parts.append((int(x1), int(y1), int(x2 - x1), int(y2 - y1)))
                out.append({"component": c, "level": lvl, "root_x": x, "root_y": y, "score": float(np.float32(rootv[y, x])),
                            "parts": np.asarray(parts, np.int32)})
    return out
