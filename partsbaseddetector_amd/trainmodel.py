"""trainmodel(): the reference's matlab/learning/trainmodel.m over the device calls (include/pbd.h) -- a
model from annotated keypoints -- and trainmodel_ref(), the same pipeline in numpy over cluster_parts_ref() and train_ref().

The pipeline (trainmodel.m): initmodel and data_def; the part types of each part by k-means on its offset to its parent
(clusterparts.m, pbd_cluster_parts on the device); one warped-positive model per (part, type) (train with warp = 1), merged per
part (mergemodels.m); the tree model assembled from them (buildmodel.m); a latent pass with every positive's types fixed to its
clusters; a latent pass with the types free.

cluster_parts_ref() is the yardstick of pbd_cluster_parts: the rules of include/pbd.h in numpy over qp.reduce_r, compared bit for
bit with the device (tests/test_gpu_cluster_parts.py).  Matlab's rand is not reproduced, so the partitions are this function's,
not Matlab's.

Project decisions: a positive's boxes are integers (point_to_box's real boxes rounded with Matlab's round)
everywhere, initmodel and data_def included; a type with one member keeps that member as its centre; max_iter exists; idx= and
part_models= replace the Matlab file cache; a type without a usable positive is an error, not an empty model.
`pa` is Matlab's parent table wherever trainmodel.m takes it (1-based, 0 for the root); the device call and cluster_parts_ref
take the 0-based `parent` (root -1).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, synth
from . import warp as W
from .model import Model
from .qp import reduce_r, reduce_seq

MAX_MIX = _lib.MAX_MIX
NEG_PART = 100            # trainmodel.m:24: the part models see the first 100 negatives
DEFW = [0.01, 0.0, 0.01, 0.0]   # buildmodel.m:66


# ---- the clustering's yardstick -----------------------------------------------------------------------------------------------
def parent_of(pa) -> np.ndarray:
    """Matlab's pa (1-based, 0 for the root) -> the 0-based parent table (root -1)"""
    return np.asarray(pa, np.int64).ravel().astype(np.int32) - 1


def _check_cluster(d, parent, K, trials, max_iter):
    if d.ndim != 3 or d.shape[2] != 2 or len(parent) != d.shape[0] or len(K) != d.shape[0]:
        raise ValueError("def is (nparts, npos, 2), parent and K (nparts,)")
    P, N = d.shape[:2]
    if P < 2 or N < 1 or trials < 1 or max_iter < 1 or P * trials > 1 << 20:
        raise ValueError(f"nparts {P} (>= 2), npos {N}, trials {trials}, max_iter {max_iter} (>= 1), at most 2^20 part x trial pairs")
    for p in range(P):
        if not 1 <= K[p] <= MAX_MIX:
            raise ValueError(f"part {p}: K {K[p]} (1..{MAX_MIX})")
        if (parent[p] != -1) if p == 0 else not 0 <= parent[p] < p:
            raise ValueError(f"part {p}: parent {parent[p]} breaks the topological order")


def offsets(d: np.ndarray, parent, p: int) -> np.ndarray:
    """X of part p (clusterparts.m:9-17): its offset to its parent; for the root its lowest-numbered child's offset to it"""
    return d[1] - d[0] if p == 0 else d[p] - d[int(parent[p])]


def anchor_of(c: float) -> int:
    """buildmodel.m:70 then zeroIndex: matlab_round(c + 1) - 1; NaN 0; saturating at the int32 range"""
    if c != c:
        return 0
    v = c + 1.0
    if math.isinf(v):
        return 2 ** 31 - 1 if v > 0 else -2 ** 31
    return int(min(max(W.matlab_round(v) - 1, -2 ** 31), 2 ** 31 - 1))


def _labels(X: np.ndarray, c: np.ndarray):
    """Matlab's [z, g] = min(D, [], 2): NaN skipped, the first minimum; a row of NaN is NaN at index 1"""
    label = np.full(len(X), -1, np.int64)
    z = np.full(len(X), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(c)):
            dx, dy = X[:, 0] - c[t, 0], X[:, 1] - c[t, 1]
            D = (0.0 + dx * dx) + dy * dy
            take = ~np.isnan(D) & ((label < 0) | (D < z))
            label[take] = t
            z[take] = D[take]
    label[label < 0] = 0
    return label, z


def _centroids(X: np.ndarray, g: np.ndarray, k: int, R):
    counts = np.bincount(g, minlength=k)[:k]
    c = np.full((k, 2), np.nan)
    for t in range(k):
        if counts[t]:
            m = g == t
            c[t] = [R(np.where(m, X[:, 0], 0.0)) / float(counts[t]), R(np.where(m, X[:, 1], 0.0)) / float(counts[t])]
    return c, counts


def k_means_ref(X: np.ndarray, start, max_iter: int, R=reduce_r):
    """one trial (k_means.m with the rules of include/pbd.h) from the centroids X[start]: (labels, centres, counts, sumdist,
    iterations)"""
    c = X[np.asarray(start, np.int64)].copy()
    g = np.full(len(X), -1, np.int64)
    it = 0
    while True:
        it += 1
        g2, z = _labels(X, c)
        changed = bool(np.any(g2 != g))
        g = g2
        c, counts = _centroids(X, g, len(c), R)
        if not changed or it >= max_iter:
            return g, c, counts, R(z), it


def pick_trial(sumdist) -> int:
    """clusterparts.m:25-26: the first trial below every earlier one, NaN never; none: trial 0"""
    best = -1
    for r, v in enumerate(sumdist):
        if v == v and (best < 0 or v < sumdist[best]):
            best = r
    return max(best, 0)


def cluster_parts_ref(deffeat, parent, K, trials: int = 100, max_iter: int = 1000, seed: int = 0, literal: bool = False) -> dict:
    """pbd_cluster_parts in numpy: the dict Handle.cluster_parts returns.  literal: sequential sums instead of R(.)"""
    d = np.ascontiguousarray(deffeat, np.float64)
    parent = np.asarray(parent, np.int64).ravel()
    K = np.asarray(K, np.int64).ravel()
    trials, max_iter = int(trials), int(max_iter)
    _check_cluster(d, parent, K, trials, max_iter)
    R = reduce_seq if literal else reduce_r
    P, N = d.shape[:2]
    start = (synth.splitmix64(int(seed), P * trials * MAX_MIX) % np.uint64(N)).astype(np.int64).reshape(P, trials, MAX_MIX)
    out = {"idx": np.zeros((P, N), np.int32), "centres": np.full((P, MAX_MIX, 2), np.nan), "counts": np.zeros((P, MAX_MIX), np.int32),
           "anchors": np.zeros((P, MAX_MIX, 2), np.int32), "info": np.zeros(P, _lib.CLUSTER_INFO_DTYPE),
           "sumdist_all": np.zeros((P, trials)), "iters_all": np.zeros((P, trials), np.int32)}
    for p in range(P):
        X = offsets(d, parent, p)
        k = int(K[p])
        runs = [k_means_ref(X, start[p, r, :k], max_iter, R) for r in range(trials)]
        out["sumdist_all"][p] = [run[3] for run in runs]
        out["iters_all"][p] = [run[4] for run in runs]
        b = pick_trial(out["sumdist_all"][p])
        g, c, counts, sd, it = runs[b]
        out["idx"][p] = g
        out["centres"][p, :k] = c
        out["counts"][p, :k] = counts
        out["info"][p] = (b, it, sd)
        if p > 0:
            out["anchors"][p, :k] = [[anchor_of(v) for v in row] for row in c]
    return out


def centres_of(deffeat, parent, idx, K) -> np.ndarray:
    """the centres (nparts, 16, 2) of given types, summed as the clustering sums them: what pbd_cluster_parts returns for the
    partition it ends in"""
    d = np.ascontiguousarray(deffeat, np.float64)
    out = np.full((d.shape[0], MAX_MIX, 2), np.nan)
    for p in range(d.shape[0]):
        out[p, :int(K[p])] = _centroids(offsets(d, parent, p), np.asarray(idx[p], np.int64), int(K[p]), reduce_r)[0]
    return out


def anchors_of(centres) -> np.ndarray:
    """(nparts, 16, 2) int32 anchors of centres; the root's are 0"""
    c = np.asarray(centres, np.float64)
    out = np.zeros(c.shape, np.int32)
    for p in range(1, c.shape[0]):
        out[p] = [[anchor_of(v) for v in row] for row in c[p]]
    return out


# ---- the pipeline's host steps ------------------------------------------------------------------------------------------------
def point_to_box(points, pa) -> np.ndarray:
    """pointtobox.m: points (npos, nparts, 2) -> real-valued boxes (npos, nparts, 4) = x1, y1, x2, y2, a square around every
    point whose side is the 0.85 quantile (Matlab's method 7 = numpy's `linear`) of the positive's limb lengths, each divided by
    exp(median over the positives of log(limb) - log(limb 1))"""
    pts = np.asarray(points, np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[1] != len(pa) or len(pa) < 2:
        raise ValueError("points is (npos, nparts, 2) with nparts = len(pa) >= 2")
    par = parent_of(pa)
    dlt = pts[:, 1:, :] - pts[:, par[1:], :]
    ln = np.sqrt(dlt[:, :, 0] * dlt[:, :, 0] + dlt[:, :, 1] * dlt[:, :, 1])          # (npos, nparts - 1)
    r = np.exp(np.median(np.log(ln) - np.log(ln[:, :1]), axis=0))
    size = np.quantile(ln / r, 0.85, axis=1)
    half = (size / 2)[:, None]
    return np.stack([pts[:, :, 0] - half, pts[:, :, 1] - half, pts[:, :, 0] + half, pts[:, :, 1] + half], axis=2)


def round_boxes(boxes) -> np.ndarray:
    """real boxes -> the integer inclusive boxes train() takes, by Matlab's round"""
    b = np.asarray(boxes, np.float64)
    return np.array([W.matlab_round(float(v)) for v in b.ravel()], np.int64).reshape(b.shape)


def with_boxes(pos, pa) -> List[dict]:
    """copies of the positives, each with integer "boxes" (nparts, 4): its own, or point_to_box's rounded"""
    if all(p.get("boxes") is not None for p in pos):
        return [dict(p, boxes=np.asarray(p["boxes"], np.int64).reshape(-1, 4)) for p in pos]
    bx = round_boxes(point_to_box([p["points"] for p in pos], pa))
    return [dict(p, boxes=np.asarray(p["boxes"], np.int64).reshape(-1, 4) if p.get("boxes") is not None else bx[i])
            for i, p in enumerate(pos)]


def _root_area(p) -> float:
    b = np.asarray(p["boxes"], np.float64).reshape(-1, 4)[0]
    return float((b[2] - b[0] + 1) * (b[3] - b[1] + 1))


def percentile_index(n: int) -> int:
    """initmodel.m:15's index into the sorted areas, 1-based: floor(0.05 n), at least 1 (Matlab's 0 for n < 20 is an error)"""
    return max(int(math.floor(n * 0.05)), 1)


def initmodel(pos, sbin: int, tsize: Optional[int] = None, interval: int = 10) -> Model:
    """initmodel.m: one part, one zero k x k x 32 filter, bias 0; k = floor(sqrt(area) / sbin) of the 5th-percentile area of
    part 0's boxes, or tsize"""
    if not len(pos):
        raise ValueError("no positives")
    if tsize is None:
        areas = np.sort([_root_area(p) for p in pos])
        k = int(math.floor(math.sqrt(float(areas[percentile_index(len(areas)) - 1])) / sbin))
    else:
        k = int(tsize)
    if k < 1:
        raise ValueError(f"filter size {k}: the part boxes are smaller than one cell of {sbin} pixels")
    return Model(name="init", interval=int(interval), thresh=0.0, sbin=int(sbin), filtersw=[np.zeros((k, k * 32))], biasw=[0.0],
                 filterid=[[[0]]], biasid=[[[0]]], defid=[[[]]], parentid=[[-1]])


def data_def(pos, k: int) -> np.ndarray:
    """data_def.m: (nparts, npos, 2), every point divided by sqrt(w h) / k of its positive's part-0 box"""
    scale = np.array([math.sqrt(_root_area(p)) / math.sqrt(float(k) * float(k)) for p in pos])
    pts = np.array([np.asarray(p["points"], np.float64).reshape(-1, 2) for p in pos])       # (npos, nparts, 2)
    return np.ascontiguousarray((pts / scale[:, None, None]).transpose(1, 0, 2))


def merge_models(models: Sequence[Model]) -> Model:
    """mergemodels.m: one component per component of every model, the parameter lists concatenated"""
    first = models[0]
    out = Model(name=first.name, interval=first.interval, thresh=first.thresh, sbin=first.sbin, norient=first.norient, flen=first.flen)
    for m in models:
        nf, nb, nd = len(out.filtersw), len(out.biasw), len(out.defw)
        out.filtersw += [np.array(f, np.float64) for f in m.filtersw]
        out.biasw += [float(b) for b in m.biasw]
        out.defw += [list(d) for d in m.defw]
        out.anchors += [tuple(a) for a in m.anchors]
        out.filterid += [[[f + nf for f in part] for part in comp] for comp in m.filterid]
        out.biasid += [[[b + nb for b in part] for part in comp] for comp in m.biasid]
        out.defid += [[[d + nd for d in part] for part in comp] for comp in m.defid]
        out.parentid += [list(comp) for comp in m.parentid]
    out.validate()
    return out


def build_model(init: Model, part_models: Sequence[Model], idx, centres_or_anchors, K, pa) -> Model:
    """buildmodel.m: the tree model of the separately trained part models.  Every bias is 0; a child's L x K biases are laid out
    base + k * L + l; filter k of part p is part model p's component k; every deformation is [0.01, 0, 0.01, 0] with the anchors
    given (integers), or those of the centres given (floats)."""
    par = parent_of(pa)
    K = [int(k) for k in K]
    a = np.asarray(centres_or_anchors)
    anchors = a if np.issubdtype(a.dtype, np.integer) else anchors_of(a)
    check_types(idx, K)
    m = Model(name="built", interval=init.interval, thresh=0.0, sbin=init.sbin, norient=init.norient, flen=init.flen)
    fid_c, bid_c, did_c = [], [], []
    for p in range(len(par)):
        if (par[p] != -1) if p == 0 else not 0 <= par[p] < p:
            raise ValueError(f"part {p}: parent {par[p]} breaks the topological order")
        pm = part_models[p]
        if pm.ncomponents() < K[p]:
            raise ValueError(f"part {p}: {pm.ncomponents()} part models for {K[p]} types")
        if p == 0:
            bid_c.append([len(m.biasw)])
            m.biasw.append(0.0)
        else:
            L, base = K[par[p]], len(m.biasw)
            m.biasw += [0.0] * (K[p] * L)
            bid_c.append([base + k * L + l for l in range(L) for k in range(K[p])])
        fid_c.append(list(range(len(m.filtersw), len(m.filtersw) + K[p])))
        m.filtersw += [np.array(pm.filtersw[pm.filterid[k][0][0]], np.float64) for k in range(K[p])]
        if p == 0:
            did_c.append([])
        else:
            did_c.append(list(range(len(m.defw), len(m.defw) + K[p])))
            m.defw += [list(DEFW) for _ in range(K[p])]
            m.anchors += [(int(anchors[p][k][0]), int(anchors[p][k][1])) for k in range(K[p])]
    m.filterid, m.biasid, m.defid, m.parentid = [fid_c], [bid_c], [did_c], [[int(v) for v in par]]
    m.validate()
    return m


def check_types(idx, K) -> None:
    for p, k in enumerate(K):
        g = np.asarray(idx[p], np.int64)
        if len(g) and (g.min() < 0 or g.max() >= k):
            raise ValueError(f"part {p}: a type outside 0..{int(k) - 1}")
        for t in range(int(k)):
            if not np.any(g == t):
                raise ValueError(f"part {p} type {t} has no positive")


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
_DEVICE_ONLY = ("device", "conv_mode")


def augmented(on_device: bool, pos, pa, augment, device: int = 0):
    """the positives multiplied by `augment` = {"degrees": (...), "mirror": perm or None} (augment.py), on
    the device or in numpy, and info["augment"]: the copies per positive and the total"""
    from . import augment as A
    unknown = set(augment) - {"degrees", "mirror"}
    if unknown:
        raise ValueError(f"augment has no key {sorted(unknown)[0]!r}")
    degrees, mirror = tuple(augment.get("degrees", ())), augment.get("mirror")
    if mirror is not None:
        mirror = A.check_mirror(mirror, pa)
    for p in pos:
        if p.get("points") is None:
            raise ValueError("augmentation maps a positive's points: every positive needs \"points\"")
    out = A.augment_positives(pos, degrees, mirror, device) if on_device else A.augment_positives_ref(pos, degrees, mirror)
    return out, {"degrees": [float(d) for d in degrees], "mirror": None if mirror is None else [int(v) for v in mirror],
                 "copies": len(A.copies(degrees, mirror)), "total": len(out)}


def _pipeline(on_device: bool, pos, neg, K, pa, sbin, tsize, trials, seed, idx, part_models, cluster_max_iter, train_kw, augment=None):
    from . import train as T
    if on_device:
        train_fn, kw = T.train, dict(train_kw)
    else:
        train_fn, kw = T.train_ref, {k: v for k, v in train_kw.items() if k not in _DEVICE_ONLY}
    kw["seed"] = int(seed)
    K = [int(k) for k in K]
    parent = parent_of(pa)
    if len(K) != len(parent):
        raise ValueError("K and pa differ in length")
    aug_info = None
    if augment is not None:
        pos, aug_info = augmented(on_device, pos, pa, augment, train_kw.get("device", 0))
    elif not on_device:
        pos = T.host_positives(pos)
    pos = with_boxes(pos, pa)
    init = initmodel(pos, sbin, tsize)
    ksize = int(init.filtersw[0].shape[0])
    deff = data_def(pos, ksize)
    info = {"def": deff, "cluster": None}
    if aug_info is not None:
        info["augment"] = aug_info
    # 1. the part types
    if idx is None:
        if on_device:
            from .detector import PartsBasedDetector
            det = PartsBasedDetector(device=train_kw.get("device", 0), dtype=train_kw.get("dtype", np.float32))
            det.distributeModel(init)
            try:
                cl = det.clusterParts(deff, parent, K, trials, cluster_max_iter, seed)
            finally:
                det.hd.close()
        else:
            cl = cluster_parts_ref(deff, parent, K, trials, cluster_max_iter, seed)
        idx, centres, info["cluster"] = cl["idx"], cl["centres"], cl
    else:
        idx = np.asarray(idx, np.int32).reshape(len(K), len(pos))
        check_types(idx, K)
        centres = centres_of(deff, parent, idx, K)
    check_types(idx, K)
    anchors = anchors_of(centres)
    info.update(idx=np.asarray(idx, np.int32), centres=centres, anchors=anchors, part_info=None)
    # 2. one warped-positive model per (part, type)
    if part_models is None:
        part_models, info["part_info"] = [], []
        for p in range(len(K)):
            models, infos = [], []
            for k in range(K[p]):
                spos = [dict(im=q["im"], boxes=np.asarray(q["boxes"], np.int64)[p:p + 1]) for n, q in enumerate(pos) if idx[p][n] == k]
                if not any(W.keeps(q["boxes"][0], ksize, int(sbin)) for q in spos):
                    raise ValueError(f"part {p} type {k} has no positive of at least {ksize * int(sbin)} x {ksize * int(sbin)} pixels")
                mk, ik = train_fn(init, spos, list(neg[:NEG_PART]), 1, **kw)
                models.append(mk)
                infos.append(ik)
            part_models.append(merge_models(models))
            info["part_info"].append(infos)
    info["part_models"] = list(part_models)
    # 3. the tree, 4. types fixed to the clusters, 5. types free
    built = build_model(init, part_models, idx, anchors, K, pa)
    fixed = [dict(im=q["im"], boxes=q["boxes"], mix=np.asarray(idx[:, n], np.int32)) for n, q in enumerate(pos)]
    model1, info["final1"] = train_fn(built, fixed, list(neg), 0, **kw)
    free = [dict(im=q["im"], boxes=q["boxes"]) for q in pos]
    model, info["final"] = train_fn(model1, free, list(neg), 0, **kw)
    info.update(built=built, model1=model1)
    return model, info


def trainmodel(pos, neg, K, pa, sbin, tsize: Optional[int] = None, trials: int = 100, seed: int = 0, idx=None, part_models=None,
               cluster_max_iter: int = 1000, augment: Optional[dict] = None, **train_kw):
    """trainmodel.m on the device: (the trained Model, info).  pos: [{"im": ndarray or device tensor, "points": (nparts, 2) pixel coordinates,
    "boxes": optional (nparts, 4) int, 0-based inclusive (absent: point_to_box, rounded)}]; neg: frames; K: types per part; pa:
    Matlab's parent table (1-based, 0 for the root); sbin: the HOG cell; tsize: the filter side (None: initmodel's).  idx
    (nparts, npos) and part_models (one merged Model per part) skip a finished stage, in place of the Matlab file cache.  A
    type with no positive, or with none of at least a filter's pixels, raises ValueError.  seed: the clustering's and every
    train()'s.  train_kw: train()'s other keywords, the same for every call.  info: def, idx, centres, anchors, cluster
    (Handle.cluster_parts' dict, None with idx=), part_models, part_info ([part][type] train() infos, None with part_models=),
    built (buildmodel's model), model1 and final1 (the fixed-type pass), final (the free pass).
    augment = {"degrees": (...), "mirror": perm or None}: every positive is first multiplied on the device into its copies
    mirror in (no, yes if a permutation of the parts is given) x degrees in (0, *degrees) (augment.augment_positives, DESIGN.md
    section 6r); the copies stay on the device, carry mapped points and no boxes (point_to_box makes them), and the unchanged
    pipeline runs on the extended list (idx= then has one column per copy).  info["augment"] = {degrees, mirror, copies (per
    positive), total}.  None: no augmentation, no such key."""
    return _pipeline(True, pos, neg, K, pa, sbin, tsize, trials, seed, idx, part_models, cluster_max_iter, train_kw, augment)


def trainmodel_ref(pos, neg, K, pa, sbin, tsize: Optional[int] = None, trials: int = 100, seed: int = 0, idx=None, part_models=None,
                   cluster_max_iter: int = 1000, augment: Optional[dict] = None, **train_kw):
    """trainmodel() in numpy: augment_positives_ref, cluster_parts_ref and train_ref on host copies (device and conv_mode
    keywords are ignored)"""
    return _pipeline(False, pos, neg, K, pa, sbin, tsize, trials, seed, idx, part_models, cluster_max_iter, train_kw, augment)
