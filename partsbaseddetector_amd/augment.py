"""Augmented training positives: rotated and mirrored copies of annotated frames.

The reference's training pipeline multiplies its positives before trainmodel sees them (matlab/globals.m:18-23 creates the
imrotate/ and imflip/ caches, matlab/learning/map_rotate_points.m maps keypoints into a rotated image, train.m:130,165 speaks of
flipped examples); the step itself, PARSE_data.m, is not in the reference.  This module states the rule once in numpy -- the
yardstick pbd_augment_frames* matches byte for byte (tests/test_gpu_augment.py) -- and builds the extended list of positives on
the device (augment_positives) or on the host (augment_positives_ref).

The rule.  A copy of a frame `im` (rows x cols [x cn], any dtype) is rotate(mirror(im)).
  mirror    column q becomes cols - 1 - q.
  rotate    degrees == 0: none, the copy has the frame's size.  Otherwise the geometry of map_rotate_points.m:20-35: (c, s) =
            (cos, sin)(degrees * pi / 180), exactly {0, +-1} for multiples of 90; hA = ((rows - 1) / 2, (cols - 1) / 2); the
            corners (-hAr, hAc), (hAr, hAc) as row vectors times [c s; -s c]; hB = ceil(max|.| / 2) * 2 per axis; the copy is
            (2 hBr + 1) x (2 hBc + 1); its pixel (R, Q) reads the source at r = (R - hBr) c + (Q - hBc) s + hAr,
            q = -((R - hBr) s) + (Q - hBc) c + hAc, every product rounded, sums left to right, index floor(x + 0.5), zero bytes
            outside: nearest neighbour (imrotate's default), positive angles counter-clockwise.
  points    (x, y), 0-based, real: x -> cols - 1 - x, then the forward map of map_rotate_points.m:40.  In a mirrored copy part
            p takes the mirrored point of part perm[p] (left and right parts swap names).
The coefficients are inputs of the yardstick (`coef`): a test feeds it pbd_augment_plan's, so no two libms have to agree.
Project decisions: imrotate's toolbox arithmetic is not reproduced (as imresize's is not, section 6k); no bilinear or cropped
rotation; boxes are not rotated -- augmentation acts on points, before point_to_box, so a copy carries "im" and "points" only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_SIDE = 32000          # a frame's largest side (include/pbd.h)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def coefficients(degrees: float) -> Tuple[float, float]:
    """(c, s) of a rotation: cos and sin of degrees * pi / 180 in double, exact for the multiples of 90"""
    d = float(degrees)
    if not math.isfinite(d):
        raise ValueError("degrees must be finite")
    if math.fmod(d, 90.0) == 0.0:
        k = int(math.fmod(d, 360.0) / 90.0) % 4
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[k]
    phi = d * math.pi / 180
    return math.cos(phi), math.sin(phi)


def _geometry(rows: int, cols: int, degrees: float, coef=None):
    """(rotate, out_rows, out_cols, c, s, hAr, hAc, hBr, hBc) of one copy"""
    rows, cols = int(rows), int(cols)
    if not (1 <= rows <= MAX_SIDE and 1 <= cols <= MAX_SIDE) or not math.isfinite(float(degrees)):
        raise ValueError(f"{rows}x{cols} (1..{MAX_SIDE}) by {degrees} degrees (finite)")
    hAr, hAc = (float(rows) - 1) / 2, (float(cols) - 1) / 2
    if float(degrees) == 0.0:
        return False, rows, cols, 1.0, 0.0, hAr, hAc, 0.0, 0.0
    c, s = (float(coef[0]), float(coef[1])) if coef is not None else coefficients(degrees)
    u0, u1, v = -hAr, hAr, hAc
    mr = max(abs(u0 * c - v * s), abs(u1 * c - v * s))
    mc = max(abs(u0 * s + v * c), abs(u1 * s + v * c))
    hBr, hBc = math.ceil(mr / 2) * 2.0, math.ceil(mc / 2) * 2.0
    return True, int(2 * hBr + 1), int(2 * hBc + 1), c, s, hAr, hAc, hBr, hBc


def plan(rows: int, cols: int, degrees: float, coef=None):
    """pbd_augment_plan in numpy: (out_rows, out_cols, (c, s)) of a rows x cols frame turned by `degrees`"""
    _, orows, ocols, c, s = _geometry(rows, cols, degrees, coef)[:5]
    return orows, ocols, (c, s)


def rotate_ref(im: np.ndarray, degrees: float, mirror: bool = False, coef=None) -> np.ndarray:
    """the copy rotate(mirror(im)) of a rows x cols [x cn] array of any dtype; coef = (c, s) replaces coefficients(degrees)"""
    im = np.asarray(im)
    if im.ndim not in (2, 3):
        raise ValueError("a frame is rows x cols or rows x cols x channels")
    src = im[:, ::-1] if mirror else im
    rot, orows, ocols, c, s, hAr, hAc, hBr, hBc = _geometry(im.shape[0], im.shape[1], degrees, coef)
    if not rot:
        return np.array(src)
    u = (np.arange(orows, dtype=np.float64) - hBr)[:, None]
    v = (np.arange(ocols, dtype=np.float64) - hBc)[None, :]
    r = np.floor(((u * c + v * s) + hAr) + 0.5)
    q = np.floor(((-(u * s) + v * c) + hAc) + 0.5)
    inside = (r >= 0) & (r < im.shape[0]) & (q >= 0) & (q < im.shape[1])
    out = np.zeros((orows, ocols) + im.shape[2:], im.dtype)
    out[inside] = src[r[inside].astype(np.int64), q[inside].astype(np.int64)]
    return out


def points_ref(xy, rows: int, cols: int, degrees: float, mirror: bool = False, coef=None) -> np.ndarray:
    """pbd_augment_points in numpy: points (n, 2) = (x, y) of a rows x cols frame mapped into its copy"""
    p = np.array(xy, np.float64).reshape(-1, 2)
    rot, _, _, c, s, hAr, hAc, hBr, hBc = _geometry(rows, cols, degrees, coef)
    x, y = p[:, 0], p[:, 1]
    if mirror:
        x = (float(cols) - 1) - x
    if rot:
        u, v = y - hAr, x - hAc
        y = (u * c - v * s) + hBr
        x = (u * s + v * c) + hBc
    return np.stack([x, y], axis=1)


def check_mirror(perm, pa) -> np.ndarray:
    """the part permutation of a mirrored copy, checked: an involution of 0..nparts-1 that maps the part tree onto itself
    (parent[perm[p]] == perm[parent[p]]; pa is Matlab's parent table, 1-based with 0 for the root).  Returns it as int64."""
    g = np.asarray(perm, np.int64).ravel()
    parent = np.asarray(pa, np.int64).ravel() - 1
    n = len(parent)
    if len(g) != n or sorted(g.tolist()) != list(range(n)):
        raise ValueError(f"mirror is a permutation of the {n} parts")
    for p in range(n):
        if g[g[p]] != p:
            raise ValueError(f"mirror is not an involution: part {p} -> {g[p]} -> {g[g[p]]}")
        want = -1 if parent[p] < 0 else g[parent[p]]
        if parent[g[p]] != want:
            raise ValueError(f"mirror breaks the tree: the parent of part {g[p]} is {parent[g[p]]}, that of part {p} maps to {want}")
    return g


def copies(degrees: Sequence[float], mirror) -> List[Tuple[bool, float]]:
    """the (mirror, degrees) of one positive's copies, in order: mirror in (no, yes if given) x degrees in (0, *degrees)"""
    degs = [0.0] + [float(d) for d in degrees]
    for d in degs:
        if not math.isfinite(d):
            raise ValueError("degrees must be finite")
    return [(m, d) for m in ((False, True) if mirror is not None else (False,)) for d in degs]


def _points_of(p) -> np.ndarray:
    return np.asarray(p["points"], np.float64).reshape(-1, 2)


def _perm_of(mirror, nparts: int):
    if mirror is None:
        return None
    g = np.asarray(mirror, np.int64).ravel()
    if len(g) != nparts or sorted(g.tolist()) != list(range(nparts)):
        raise ValueError(f"mirror is a permutation of the {nparts} parts")
    return g


def augment_positives_ref(pos, degrees: Sequence[float], mirror=None, coef_of=None) -> List[dict]:
    """the extended list in numpy: for every positive {"im", "points"} its copies in copies()' order, each {"im": ndarray,
    "points": (nparts, 2)}.  coef_of(degrees) -> (c, s) replaces coefficients (a test passes pbd_augment_plan's)."""
    out = []
    for p in pos:
        im = np.asarray(p["im"].cpu().numpy() if hasattr(p["im"], "cpu") else p["im"])
        pts = _points_of(p)
        perm = _perm_of(mirror, len(pts))
        for m, d in copies(degrees, mirror):
            coef = coef_of(d) if coef_of is not None and d != 0 else None
            out.append({"im": rotate_ref(im, d, m, coef),
                        "points": points_ref(pts[perm] if m else pts, im.shape[0], im.shape[1], d, m, coef)})
    return out


# ---- on the device ----------------------------------------------------------------------------------------------------------
def plan_c(rows: int, cols: int, degrees: float):
    """pbd_augment_plan: (out_rows, out_cols, (c, s)) -- the coefficients the kernel uses"""
    from . import _lib
    lib = _lib.load()
    r, c, coef = C.c_int(), C.c_int(), (C.c_double * 2)()
    rc = lib.pbd_augment_plan(int(rows), int(cols), float(degrees), C.byref(r), C.byref(c), coef)
    if rc != _lib.PBD_OK:
        raise _lib.PbdError(rc, lib.pbd_last_error(None).decode())
    return r.value, c.value, (coef[0], coef[1])


def points_c(xy, rows: int, cols: int, degrees: float, mirror: bool = False) -> np.ndarray:
    """pbd_augment_points: points (n, 2) = (x, y) of a rows x cols frame mapped into its copy"""
    from . import _lib
    lib = _lib.load()
    p = np.ascontiguousarray(np.array(xy, np.float64).reshape(-1, 2))
    out = np.zeros_like(p)
    rc = lib.pbd_augment_points(int(rows), int(cols), float(degrees), 1 if mirror else 0, len(p), _lib.opt_ptr(p), _lib.opt_ptr(out))
    if rc != _lib.PBD_OK:
        raise _lib.PbdError(rc, lib.pbd_last_error(None).decode())
    return out


def augment_positives(pos, degrees: Sequence[float], mirror=None, device: int = 0) -> List[dict]:
    """the extended list on the device: as augment_positives_ref, with every "im" a torch tensor on cuda:`device` made by
    pbd_augment_frames_device (one launch per dtype and channel count among the positives) and the points mapped by
    pbd_augment_points.  Positives may be numpy arrays (uploaded once) or device tensors."""
    from .detector import PartsBasedDetector
    from .model import synthetic_tiny_model
    cps = copies(degrees, mirror)
    groups = {}
    for n, p in enumerate(pos):
        im = p["im"]
        key = (str(im.dtype).replace("torch.", ""), 1 if im.ndim == 2 else int(im.shape[2]))
        groups.setdefault(key, []).append(n)
    ims: List[Optional[object]] = [None] * (len(pos) * len(cps))
    det = PartsBasedDetector(device=device)
    det.distributeModel(synthetic_tiny_model())      # a handle needs a model; the augment call reads none of it
    try:
        for idx in groups.values():
            jobs = [(f, m, d) for f in range(len(idx)) for m, d in cps]
            got = det.augmentFrames([pos[n]["im"] for n in idx], jobs)
            for f, n in enumerate(idx):
                ims[n * len(cps):(n + 1) * len(cps)] = got[f * len(cps):(f + 1) * len(cps)]
    finally:
        det.hd.close()
    out = []
    for n, p in enumerate(pos):
        pts = _points_of(p)
        perm = _perm_of(mirror, len(pts))
        rows, cols = int(p["im"].shape[0]), int(p["im"].shape[1])
        for k, (m, d) in enumerate(cps):
            out.append({"im": ims[n * len(cps) + k], "points": points_c(pts[perm] if m else pts, rows, cols, d, m)})
    return out
