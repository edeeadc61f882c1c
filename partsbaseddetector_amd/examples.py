"""Training examples of detections, restated in numpy: the yardstick of pbd_examples* (include/pbd.h).

An example is the block-sparse feature vector the reference's Matlab training code writes for a detection
(matlab/detection/detect.m backtrack + qp_write): per part a bias block, a deformation block (children) and the feature window
under the part's filter, each at its place in the model vector, so that ``w . x`` reproduces the score.

Nothing here runs on the GPU.  The walk reads back-pointer maps in the layout ``oracle.dp_min`` returns them (Ix, Iy already
composed as the reference composes them, Ik, rooti), so the oracle's dynamic program is the reference for the walk.

The arg-max walk (pbd_set_walk, PBD_WALK_ARGMAX) needs the two passes' own pointers, which ``oracle.dp_min`` does not return:
``raw_maps`` restates DynamicProgram::min over ``oracle.dt`` called one row and one column at a time (a length-1 pass is the
identity), and ``compose`` puts the reference's composition back so that the restatement is pinned on ``oracle.dp_min`` itself.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

FLEN = 32


# ---- the model vector ---------------------------------------------------------------------------------------------------
def vector_offsets(flat) -> Tuple[int, int, int]:
    """(offset of the deformations, offset of the filters, length) of ``flat``'s model vector"""
    fbase = len(flat.biasw) + 4 * len(flat.defw)
    n = fbase
    for f in range(flat.nfilters):
        n = max(n, fbase + int(flat.filter_offset[f]) + int(flat.filter_ksize[f]) ** 2 * flat.flen)
    return len(flat.biasw), fbase, n


def model_vector(flat, dtype=np.float32) -> np.ndarray:
    """w = [biasw | defw (ndefs x 4) | filters at filter_offset], in T (pbd_model_vector)"""
    dbase, fbase, n = vector_offsets(flat)
    w = np.zeros(n, dtype)
    w[:dbase] = flat.biasw
    w[dbase:fbase] = np.asarray(flat.defw, np.float32).ravel()
    filters = flat.filters_f32 if np.dtype(dtype) == np.float32 else flat.filters_f64
    for f in range(flat.nfilters):
        o, sz = int(flat.filter_offset[f]), int(flat.filter_ksize[f]) ** 2 * flat.flen
        w[fbase + o:fbase + o + sz] = filters[o:o + sz]
    return w


def model_from_vector(model, w: np.ndarray):
    """the Model whose vector is w: a copy of ``model`` with biasw, defw and the filters taken from w (the inverse of
    model_vector of the same dtype; biases and deformations are rounded to float, as the model holds them).  The filters become
    w's values: from a float32 vector of a model whose filters carry float64 precision, the model's filters_f64 are NOT given
    back (they are the float32 values); from a float64 vector both filters_f32 and filters_f64 are."""
    import copy
    flat = model.flatten()
    dbase, fbase, n = vector_offsets(flat)
    w = np.asarray(w)
    if w.ndim != 1 or len(w) != n:
        raise ValueError(f"model vector of {len(w) if w.ndim == 1 else w.shape} values, this model's has {n}")
    out = copy.deepcopy(model)
    out.biasw = [float(v) for v in np.asarray(w[:dbase], np.float32)]
    out.defw = [[float(v) for v in row] for row in np.asarray(w[dbase:fbase], np.float32).reshape(-1, 4)]
    out.filtersw = []
    for f in range(flat.nfilters):
        k = int(flat.filter_ksize[f])
        o = fbase + int(flat.filter_offset[f])
        out.filtersw.append(np.asarray(w[o:o + k * k * flat.flen], np.float64).reshape(k, k * flat.flen))
    out.validate()
    return out


# ---- strides and walk ---------------------------------------------------------------------------------------------------
def strides(flat) -> Tuple[int, int]:
    """(hdr_words, values) of an example (pbd_example_stride)"""
    hdr_words = 4 + 2 * (3 * flat.max_parts - 1)
    vmax = 0
    for c in range(flat.ncomponents):
        v = 0
        for gp in range(flat.part_offset[c], flat.part_offset[c + 1]):
            kmax = max(int(flat.filter_ksize[flat.filterid[gm]]) for gm in range(flat.mix_offset[gp], flat.mix_offset[gp + 1]))
            v += 1 + (4 if gp > flat.part_offset[c] else 0) + kmax * kmax * flat.flen
        vmax = max(vmax, v)
    return hdr_words, (vmax + 3) // 4 * 4


def walk(flat, c: int, x: int, y: int, Ix, Iy, Ik, rooti, argmax: bool = False) -> List[Tuple[int, int, int]]:
    """(x, y, mixture) of every part of component c from the root at (x, y): src/DynamicProgram.cpp:218-244 on the maps of
    oracle.dp_min (composed Ix / Iy, Ik per pointer slot; rooti of the component).  argmax: Ix / Iy are raw_maps' IxRaw / IyRaw
    (one plane per global mixture) and a child sits where its score was taken: y = IyRaw[k][py][px], x = IxRaw[k][y][px] with
    k the plane of the winning mixture (the column pass ran over the row pass's output, so its pointer comes first)"""
    p0 = int(flat.part_offset[c])
    out = []
    for p in range(int(flat.part_offset[c + 1]) - p0):
        if p == 0:
            out.append((x, y, int(rooti[y, x])))
            continue
        px, py, pm = out[int(flat.parentid[p0 + p])]
        s = int(flat.ptr_slot[p0 + p]) + pm
        m = int(Ik[s, py, px])
        if argmax:
            k = int(flat.mix_offset[p0 + p]) + m
            cy = int(Iy[k, py, px])
            out.append((int(Ix[k, cy, px]), cy, m))
        else:
            out.append((int(Ix[s, py, px]), int(Iy[s, py, px]), m))
    return out


_walk = walk   # for the functions below whose `walk` argument names the mode


def dt_raw(oracle, score: np.ndarray, ax, bx, ay, by, osx: int, osy: int, readout: str = "reference", nan_isect=None):
    """(out, IxRaw, IyRaw) of one distance transform: the row pass as 1 x N transforms of the oracle (osy = 0: the length-1
    column pass is the identity a 0 + b 0 + src), then the column pass as M x 1 transforms of the row pass's output (osx = 0).
    They are what M + N calls of oracle.dt on those lines return, made on the lines in place through the oracle's library under
    one setting of the rule, so that a plane costs two passes and not M + N trips through oracle.dt.  readout is the oracle's
    read-out rule ("reference" or "max": include/pbd.h, pbd_dp_min, "Non-finite scores"); nan_isect, a one-element list, has
    the NaN intersections the oracle counted in these transforms added to it."""
    import ctypes as C
    lib = oracle.lib()
    dtype = score.dtype
    score = np.ascontiguousarray(score)
    M, N = score.shape
    fn = lib.pbdo_dt_f32 if dtype == np.float32 else lib.pbdo_dt_f64
    size = score.itemsize
    a = [C.c_double(v) for v in (ax, bx, ay, by)]
    tmp = np.empty((M, N), dtype)
    IxRaw = np.empty((M, N), np.int32)
    unused = np.empty(max(M, N), np.int32)
    outT = np.empty((N, M), dtype)
    IyRawT = np.empty((N, M), np.int32)
    vp, up = C.c_void_p, unused.ctypes.data
    lib.pbdo_set_dt_readout(oracle.READOUTS[readout])
    lib.pbdo_nan_isect_reset()
    try:
        s0, t0, x0 = score.ctypes.data, tmp.ctypes.data, IxRaw.ctypes.data
        for m in range(M):
            fn(vp(s0 + m * N * size), 1, N, a[0], a[1], a[2], a[3], osx, 0, vp(t0 + m * N * size), vp(x0 + m * N * 4), vp(up))
        tmpT = np.ascontiguousarray(tmp.T)
        s0, t0, y0 = tmpT.ctypes.data, outT.ctypes.data, IyRawT.ctypes.data
        for n in range(N):
            fn(vp(s0 + n * M * size), M, 1, a[0], a[1], a[2], a[3], 0, osy, vp(t0 + n * M * size), vp(up), vp(y0 + n * M * 4))
        if nan_isect is not None:
            nan_isect[0] += oracle.nan_isect()
    finally:
        lib.pbdo_set_dt_readout(oracle.READOUTS["reference"])
    return np.ascontiguousarray(outT.T), IxRaw, np.ascontiguousarray(IyRawT.T)


def raw_maps(flat, c: int, resp: np.ndarray, readout: str = "reference"):
    """DynamicProgram::min of component c on one level's responses (nfilters, H, W) of T, restated in numpy
    (src/DynamicProgram.cpp:83-171): parts in descending order, a distance transform per child mixture (dt_raw), reduceMax
    over the child's mixtures with strict > from -inf (one mixture: a copy), and parent += max into the parent's plane, kept per
    filter id as the reference keeps it.  Returns IxRaw, IyRaw (totmix, H, W: one plane per global mixture, the two passes' own
    pointers), Ik (nslots, H, W), rootv, rooti.  readout: the transform's read-out rule, as dt_raw takes it"""
    from oracle import oracle
    T = resp.dtype.type
    _, H, W = resp.shape
    p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
    totmix = int(flat.mix_offset[-1])
    IxRaw = np.zeros((totmix, H, W), np.int32)
    IyRaw = np.zeros((totmix, H, W), np.int32)
    Ik = np.zeros((max(flat.nslots, 1), H, W), np.int32)
    nc = {}
    for gp in range(p1 - 1, p0, -1):
        g0, g1 = int(flat.mix_offset[gp]), int(flat.mix_offset[gp + 1])
        gpar = p0 + int(flat.parentid[gp])
        sc = []
        for gm in range(g0, g1):
            f, d = int(flat.filterid[gm]), int(flat.defid[gm])
            w = [float(v) for v in flat.defw[d]]
            o, IxRaw[gm], IyRaw[gm] = dt_raw(oracle, np.ascontiguousarray(nc.get(f, resp[f])), -w[0], -w[1], -w[2], -w[3],
                                             int(flat.anchors[d][0]), int(flat.anchors[d][1]), readout=readout)
            sc.append(o)
        for pm in range(int(flat.mix_offset[gpar + 1]) - int(flat.mix_offset[gpar])):
            fp = int(flat.filterid[int(flat.mix_offset[gpar]) + pm])
            if fp not in nc:
                nc[fp] = np.array(resp[fp], copy=True)
            if g1 - g0 == 1:
                v = sc[0] + T(flat.biasw[int(flat.biasid[g0]) + pm])
                best = np.zeros((H, W), np.int32)
            else:
                v = np.full((H, W), -np.inf, resp.dtype)
                best = np.zeros((H, W), np.int32)
                for mm in range(g1 - g0):
                    wv = sc[mm] + T(flat.biasw[int(flat.biasid[g0 + mm]) + pm])
                    t = wv > v
                    best[t] = mm
                    v = np.where(t, wv, v)
            Ik[int(flat.ptr_slot[gp]) + pm] = best
            nc[fp] = nc[fp] + v
    g0, g1 = int(flat.mix_offset[p0]), int(flat.mix_offset[p0 + 1])
    bias = T(flat.biasw[int(flat.biasid[g0])])
    plane = lambda gm: nc.get(int(flat.filterid[gm]), resp[int(flat.filterid[gm])])
    if g1 - g0 == 1:
        rootv, rooti = plane(g0) + bias, np.zeros((H, W), np.int32)
    else:
        rootv, rooti = np.full((H, W), -np.inf, resp.dtype), np.zeros((H, W), np.int32)
        for mm in range(g1 - g0):
            wv = plane(g0 + mm) + bias
            t = wv > rootv
            rooti[t] = mm
            rootv = np.where(t, wv, rootv)
    return IxRaw, IyRaw, Ik, rootv.astype(resp.dtype), rooti


def compose(flat, c: int, IxRaw, IyRaw, Ik):
    """the Ix, Iy (nslots, H, W) oracle.dp_min returns, from raw_maps' planes: the winning mixture's IxRaw, and the reference's
    composition Iy[y][x] = IyRaw[y][Ix[y][x]] (include/DistanceTransform.hpp:233-244)"""
    Ix, Iy = np.zeros_like(Ik), np.zeros_like(Ik)
    H = Ik.shape[1]
    rows = np.arange(H)[:, None]
    p0 = int(flat.part_offset[c])
    for gp in range(p0 + 1, int(flat.part_offset[c + 1])):
        gpar = p0 + int(flat.parentid[gp])
        for pm in range(int(flat.mix_offset[gpar + 1]) - int(flat.mix_offset[gpar])):
            s = int(flat.ptr_slot[gp]) + pm
            k = int(flat.mix_offset[gp]) + Ik[s]
            Ix[s] = np.take_along_axis(IxRaw, k[None], 0)[0]
            Iy[s] = IyRaw[k, rows, Ix[s]]
    return Ix, Iy


def window(feat: np.ndarray, x: int, y: int, k: int, flen: int = FLEN) -> np.ndarray:
    """the k x k x flen window the convolution read for the response at (x, y), cells x - k/2 .., y - k/2 ..; cells outside the
    map hold the border values 0 (channels 0..flen-2) and 1 (channel flen-1)"""
    H, W = feat.shape[0], feat.shape[1] // flen
    f3 = feat.reshape(H, W, flen)
    out = np.zeros((k, k, flen), feat.dtype)
    out[:, :, flen - 1] = 1
    x0, y0 = x - k // 2, y - k // 2
    ya, yb, xa, xb = max(y0, 0), min(y0 + k, H), max(x0, 0), min(x0 + k, W)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = f3[ya:yb, xa:xb]
    return out.ravel()


def example(flat, feat: np.ndarray, c: int, placement, index: int, dtype=np.float32) -> Tuple[np.ndarray, np.ndarray]:
    """(hdr, values) of one example: the header {index, c, nblocks, nvalues, (offset, length) ...} padded with 0 to the
    stride, and the blocks' values (nvalues of them; the rest of the stride 0)"""
    hdr_words, vstride = strides(flat)
    dbase, fbase, _ = vector_offsets(flat)
    p0 = int(flat.part_offset[c])
    blocks, vals = [], []
    for p, (x, y, m) in enumerate(placement):
        gp = p0 + p
        gm = int(flat.mix_offset[gp]) + m
        if p == 0:
            blocks.append((int(flat.biasid[flat.mix_offset[gp]]), 1))
        else:
            pm = placement[int(flat.parentid[gp])][2]
            blocks.append((int(flat.biasid[gm]) + pm, 1))
        vals.append(np.ones(1, dtype))
        if p > 0:
            px, py, _ = placement[int(flat.parentid[gp])]
            d = int(flat.defid[gm])
            dx, dy = px + int(flat.anchors[d][0]) - x, py + int(flat.anchors[d][1]) - y
            blocks.append((dbase + 4 * d, 4))
            vals.append(np.array([-(dx * dx), -dx, -(dy * dy), -dy], dtype))
        f = int(flat.filterid[gm])
        k = int(flat.filter_ksize[f])
        blocks.append((fbase + int(flat.filter_offset[f]), k * k * flat.flen))
        vals.append(window(feat, x, y, k, flat.flen).astype(dtype))
    hdr = np.zeros(hdr_words, np.int32)
    v = np.concatenate(vals)
    hdr[:4] = (index, c, len(blocks), len(v))
    hdr[4:4 + 2 * len(blocks)] = np.asarray(blocks, np.int32).ravel()
    out = np.zeros(vstride, dtype)
    out[:len(v)] = v
    return hdr, out


# ---- using examples -----------------------------------------------------------------------------------------------------
def blocks(hdr: np.ndarray):
    """[(offset in w, first value, length)] of one header"""
    out, pos = [], 0
    for b in range(int(hdr[2])):
        off, ln = int(hdr[4 + 2 * b]), int(hdr[5 + 2 * b])
        out.append((off, pos, ln))
        pos += ln
    return out


def dot(hdr: np.ndarray, values: np.ndarray, w: np.ndarray) -> np.ndarray:
    """w . x of every example in float64 (a block repeated at one offset counts twice, as the score did)"""
    hdr = np.atleast_2d(hdr)
    values = np.atleast_2d(values)
    w = np.asarray(w, np.float64)
    out = np.zeros(len(hdr))
    for i, h in enumerate(hdr):
        out[i] = sum(float(np.dot(w[o:o + n], np.asarray(values[i, s:s + n], np.float64))) for o, s, n in blocks(h))
    return out


def abs_dot(hdr: np.ndarray, values: np.ndarray, w: np.ndarray) -> np.ndarray:
    """sum |w_i x_i| of every example in float64 (the scale of the rounding bound of DESIGN.md section 6h)"""
    return dot(hdr, np.abs(np.asarray(values, np.float64)), np.abs(np.asarray(w, np.float64)))


def densify(hdr: np.ndarray, values: np.ndarray, n: int) -> np.ndarray:
    """(examples, n) float64 dense feature vectors (repeated blocks added)"""
    hdr = np.atleast_2d(hdr)
    values = np.atleast_2d(values)
    out = np.zeros((len(hdr), n))
    for i, h in enumerate(hdr):
        for o, s, ln in blocks(h):
            out[i, o:o + ln] += values[i, s:s + ln]
    return out


def rounding_bound(flat, hdr: np.ndarray, values: np.ndarray, w: np.ndarray, dtype=np.float32) -> np.ndarray:
    """(k^2 flen + 3 nparts + 8) u sum|w_i x_i| per example: recursive summation of one filter's products plus the dynamic
    program's adds, u = 2^-24 (float) or 2^-53 (double); k is the largest filter of the model"""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    k = int(np.max(flat.filter_ksize))
    return (k * k * flat.flen + 3 * flat.max_parts + 8) * u * abs_dot(hdr, values, w)


def placement_score(flat, resp: np.ndarray, c: int, placement) -> float:
    """the score of a placement in float64 from one level's responses (nfilters, H, W) of T: the parts' responses, the biases
    the dynamic program added and the deformation terms at the placement's displacements"""
    p0 = int(flat.part_offset[c])
    s = 0.0
    for p, (x, y, m) in enumerate(placement):
        gp = p0 + p
        gm = int(flat.mix_offset[gp]) + m
        s += float(resp[int(flat.filterid[gm]), y, x])
        if p == 0:
            s += float(flat.biasw[flat.biasid[flat.mix_offset[gp]]])
            continue
        px, py, pm = placement[int(flat.parentid[gp])]
        d = int(flat.defid[gm])
        dx, dy = px + int(flat.anchors[d][0]) - x, py + int(flat.anchors[d][1]) - y
        w = [float(v) for v in flat.defw[d]]
        s += float(flat.biasw[int(flat.biasid[gm]) + pm]) - (w[0] * dx * dx + w[1] * dx + w[2] * dy * dy + w[3] * dy)
    return s


def _features_pyramid(flat, im, dtype, fine: bool):
    """the oracle's level list, or with the fine octave in front of it (fineoctave.py): levels then index the longer list"""
    from oracle import oracle
    if not fine:
        return oracle.features_pyramid(flat, im, dtype)
    from .fineoctave import features_pyramid
    return features_pyramid(flat, im, dtype, True)


class FrameMaps:
    """the oracle's features, responses and per-component DP maps of one frame (computed on first use per level)"""

    def __init__(self, flat, im: np.ndarray, dtype=np.float32, walk: str = "reference", pad=(0, 0), fine: bool = False):
        from oracle import oracle
        self.oracle, self.flat, self.dtype, self.walk = oracle, flat, dtype, walk
        self.feats, self.scales = _features_pyramid(flat, im, dtype, fine)
        if tuple(pad) != (0, 0):   # the padded pyramid (padding.py): every map below follows the padded planes
            from .padding import pad_features
            self.feats = [pad_features(f, pad[0], pad[1], flat.flen) for f in self.feats]
        self._resp, self._dp = {}, {}

    def resp(self, level: int) -> np.ndarray:
        if level not in self._resp:
            self._resp[level] = self.oracle.responses(self.flat, self.feats[level])
        return self._resp[level]

    def dp(self, level: int, c: int, walk: str = "reference"):
        """oracle.dp_min's maps, or for walk "argmax" raw_maps' (IxRaw, IyRaw in place of Ix, Iy)"""
        key = (level, c, walk == "argmax")
        if key not in self._dp:
            fn = raw_maps if walk == "argmax" else self.oracle.dp_min
            self._dp[key] = fn(self.flat, c, self.resp(level))
        return self._dp[key]

    def placement(self, level: int, c: int, x: int, y: int, walk: str = None):
        walk = self.walk if walk is None else walk
        Ix, Iy, Ik, _, rooti = self.dp(level, c, walk)
        return _walk(self.flat, c, x, y, Ix, Iy, Ik, rooti, argmax=walk == "argmax")


def examples_of_records(flat, frames: Sequence[FrameMaps], records: np.ndarray, frame_offset: int = 0, dtype=np.float32,
                        walk: str = None):
    """(hdr, values) of records (n, stride) int32 as pbd_examples returns them; frames[f] holds the oracle's maps of frame f;
    walk "reference" / "argmax" (None: each frame's own mode)"""
    hdr_words, vstride = strides(flat)
    records = np.atleast_2d(np.asarray(records, np.int32))
    H = np.zeros((len(records), hdr_words), np.int32)
    V = np.zeros((len(records), vstride), dtype)
    for i, r in enumerate(records):
        fm = frames[int(r[0]) - frame_offset]
        lvl, c, x, y = int(r[2]), int(r[1]), int(r[3]), int(r[4])
        H[i], V[i] = example(flat, fm.feats[lvl], c, fm.placement(lvl, c, x, y, walk), i, dtype)
    return H, V


# ---- latent positives (pbd_detect_latent) -------------------------------------------------------------------------------
MASKED = -1e10   # Matlab's -INF, finite


def unique_model(model):
    """a copy of ``model`` in which every (component, part, mixture) has a filter of its own, in global mixture order (the mask
    of a latent search belongs to the (component, part, mixture), so shared filter ids are copied)"""
    import copy
    out = copy.deepcopy(model)
    out.filtersw, out.filterid = [], []
    for c in range(model.ncomponents()):
        fc = []
        for p in range(model.nparts(c)):
            ids = []
            for f in model.filterid[c][p]:
                ids.append(len(out.filtersw))
                out.filtersw.append(np.array(model.filtersw[f], copy=True))
            fc.append(ids)
        out.filterid.append(fc)
    out.validate()
    return out


def round_mul(a, s, dtype):
    """cv::Point_<int> * T: the product in T rounded half to even (cvRound), element-wise"""
    t = np.dtype(dtype).type
    return np.rint(t(a) * t(s)).astype(np.int64)


def part_rects(x, y, k, scale, dtype, pad=(0, 0)):
    """the record rectangle of a part of size k at (x, y) (src/DynamicProgram.cpp:238-241) as inclusive corners x1, y1, x2, y2;
    pad: (padx, pady) of a padded pyramid, (x, y) being plane coordinates (padding.py)"""
    x1, y1 = round_mul(np.asarray(x) - pad[0] - 1, scale, dtype), round_mul(np.asarray(y) - pad[1] - 1, scale, dtype)
    x2, y2 = x1 + round_mul(k, scale, dtype) - 1, y1 + round_mul(k, scale, dtype) - 1
    return np.minimum(x1, x2), np.minimum(y1, y2), np.maximum(x1, x2), np.maximum(y1, y2)


def overlap_passes(rect, box, overlap):
    """testoverlap in double with inclusive areas: inter / (area + barea - inter) > overlap (element-wise over rect's arrays)"""
    rx1, ry1, rx2, ry2 = rect
    iw = np.maximum(0, np.minimum(rx2, box[2]) - np.maximum(rx1, box[0]) + 1).astype(np.float64)
    ih = np.maximum(0, np.minimum(ry2, box[3]) - np.maximum(ry1, box[1]) + 1).astype(np.float64)
    inter = iw * ih
    area = (rx2 - rx1 + 1).astype(np.float64) * (ry2 - ry1 + 1).astype(np.float64)
    barea = float(box[2] - box[0] + 1) * float(box[3] - box[1] + 1)
    return inter / (area + barea - inter) > overlap


def mask_responses(uflat, resp, scale, boxes, overlap, mixtures=None, dtype=np.float32, pad=(0, 0)):
    """the latent mask of one level's responses (F', H, W) of the unique model: a (part, mixture) plane keeps its value only where
    the mixture is allowed and the part's record rectangle passes the overlap test with the frame's box of that part"""
    out = np.array(resp, copy=True)
    _, H, W = resp.shape
    ys, xs = np.mgrid[0:H, 0:W]
    for c in range(uflat.ncomponents):
        for gp in range(uflat.part_offset[c], uflat.part_offset[c + 1]):
            p = gp - int(uflat.part_offset[c])
            for m, gm in enumerate(range(uflat.mix_offset[gp], uflat.mix_offset[gp + 1])):
                k = int(uflat.filter_ksize[uflat.filterid[gm]])
                keep = overlap_passes(part_rects(xs, ys, k, scale, dtype, pad), boxes[p], overlap)
                if mixtures is not None and mixtures[p] >= 0 and mixtures[p] != m:
                    keep[:] = False
                out[int(uflat.filterid[gm])][~keep] = np.dtype(dtype).type(MASKED)
    return out


def latent_search(model, im: np.ndarray, boxes, overlap: float, mixtures=None, dtype=np.float32, walk: str = "reference",
                  pad=(0, 0), fine: bool = False):
    """the latent positive of one frame (pbd_detect_latent): dict(level, component, root_x, root_y, score (float), parts
    (nparts, 4) x, y, w, h, placement [(x, y, mixture)], found), walked through the oracle's maps of the masked responses of the
    unique model (walk "argmax": raw_maps' of the best level and component); ties go to the first in (level, component, y, x)
    order.  pad: (padx, pady) of a padded pyramid (padding.py): root_x / root_y and the placement are plane coordinates.  fine: the
    level list with the fine octave in front (fineoctave.py)"""
    from oracle import oracle
    from .padding import pad_features
    uflat = unique_model(model).flatten()
    feats, scales = _features_pyramid(uflat, im, dtype, fine)
    best = None
    for lvl, feat in enumerate(feats):
        feat = pad_features(feat, pad[0], pad[1], uflat.flen)
        if feat.size == 0:
            continue
        resp = mask_responses(uflat, oracle.responses(uflat, feat), scales[lvl], boxes, overlap, mixtures, dtype, pad)
        for c in range(uflat.ncomponents):
            Ix, Iy, Ik, rootv, rooti = oracle.dp_min(uflat, c, resp)
            i = int(np.argmax(rootv))       # first maximum in raster order
            if best is None or rootv.flat[i] > best[0]:
                best = (rootv.flat[i], lvl, c, i % rootv.shape[1], i // rootv.shape[1], (Ix, Iy, Ik, rooti), resp)
    v, lvl, c, x, y, maps, resp = best
    if walk == "argmax":
        IxRaw, IyRaw, Ik, _, rooti = raw_maps(uflat, c, resp)
        pl = _walk(uflat, c, x, y, IxRaw, IyRaw, Ik, rooti, argmax=True)
    else:
        pl = _walk(uflat, c, x, y, *maps)
    parts = []
    for p, (px, py, m) in enumerate(pl):
        gm = int(uflat.mix_offset[uflat.part_offset[c] + p]) + m
        x1, y1, x2, y2 = part_rects(px, py, int(uflat.filter_ksize[uflat.filterid[gm]]), scales[lvl], dtype, pad)
        parts.append((int(x1), int(y1), int(x2 - x1), int(y2 - y1)))
    score = float(np.float32(v))
    return {"level": lvl, "component": c, "root_x": x, "root_y": y, "score": score, "parts": np.asarray(parts, np.int32),
            "placement": pl, "found": score > -5e9}
