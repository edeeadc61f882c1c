"""Numpy yardstick of the model-testing calls (include/pbd.h: pbd_part_nms, pbd_best_overlap, pbd_eval_pck, pbd_eval_apk):
the reference's matlab/detection/nms.m, bestoverlap.m and matlab/evaluation/eval_pck.m, eval_apk.m, VOCap.m as plain loops
over candidate records.  Nothing here runs on the GPU; the device kernels (csrc/pbd_kernels_eval.hip) are compared with these
functions byte for byte (tests/test_gpu_eval.py), and these with a literal restatement of the .m files (tests/test_eval_cpu.py).

Records are (n, stride) int32 as Handle.pack_candidates lays them out: word 0 = frame, word 5 = the float32 score's bits, part j
at words 8 + 4 j = x, y, w, h.  Every record is read with the model's part count `nparts` (Matlab's box matrix has one width).
All arithmetic is float64, one rounding per operation, in the order written.
"""
from __future__ import annotations

import numpy as np

MAX_BOXES = 1000   # nms.m's constant


def scores(rec: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rec[:, 5]).view(np.float32)


def corners(rec: np.ndarray, nparts: int) -> np.ndarray:
    """(n, nparts, 4) float64 x1, y1, x2, y2 of every part: x1 = x, y1 = y, x2 = x + w, y2 = y + h (the two points the
    reference built the cv::Rect from, src/DynamicProgram.cpp:238-242)"""
    b = rec[:, 8:8 + 4 * nparts].reshape(len(rec), nparts, 4).astype(np.float64)
    out = b.copy()
    out[:, :, 2] = b[:, :, 0] + b[:, :, 2]
    out[:, :, 3] = b[:, :, 1] + b[:, :, 3]
    return out


def centres(rec: np.ndarray, nparts: int) -> np.ndarray:
    """(n, nparts, 2) float64 part centres (.5 x1 + .5 x2, .5 y1 + .5 y2)"""
    c = corners(rec, nparts)
    return np.stack([.5 * c[:, :, 0] + .5 * c[:, :, 2], .5 * c[:, :, 1] + .5 * c[:, :, 3]], axis=2)


def _min(a, b):     # the one definition of min / max the calls use (no NaN rule beyond IEEE's comparisons)
    return b if b < a else a


def _max(a, b):
    return b if b > a else a


def score_order(s: np.ndarray) -> list:
    """indices by score descending, ties in list order, NaN last in list order (-0.0 == +0.0): Matlab's stable
    sort(s, 'descend') with the project's NaN rule (post_ahead of the suppression stage)"""
    s = np.asarray(s, np.float32)
    idx = list(range(len(s)))
    nan = [i for i in idx if s[i] != s[i]]
    rest = [i for i in idx if s[i] == s[i]]
    rest.sort(key=lambda i: -float(s[i]))          # list.sort is stable; -(-0.0) == -(+0.0)
    return rest + nan


def pick_order(s: np.ndarray) -> list:
    """nms.m's `[vals, I] = sort(s)` taken from the end: the highest score first, among equal scores the LAST in the list
    first; NaN scores last, in list order"""
    s = np.asarray(s, np.float32)
    idx = list(range(len(s)))
    nan = [i for i in idx if s[i] != s[i]]
    rest = [i for i in idx if s[i] == s[i]]
    rest.sort(key=lambda i: float(s[i]))           # ascending, stable
    return rest[::-1] + nan


def nms_boxes(rec: np.ndarray, nparts: int) -> tuple:
    """boxes b = 0 .. nparts of every record (its parts, then the hull min x1, min y1, max x2, max y2) and their inclusive
    areas (x2 - x1 + 1) * (y2 - y1 + 1): (n, nparts + 1, 4), (n, nparts + 1)"""
    c = corners(rec, nparts)
    hull = np.stack([c[:, :, 0].min(1), c[:, :, 1].min(1), c[:, :, 2].max(1), c[:, :, 3].max(1)], axis=1)
    box = np.concatenate([c, hull[:, None, :]], axis=1)
    with np.errstate(all="ignore"):
        area = (box[:, :, 2] - box[:, :, 0] + 1.0) * (box[:, :, 3] - box[:, :, 1] + 1.0)
    return box, area


def _vmin(a, b):    # _min / _max over arrays
    return np.where(b < a, b, a)


def _vmax(a, b):
    return np.where(b > a, b, a)


def covers(box_i, area_i, box_j, overlap: float) -> np.ndarray:
    """does pick i remove each j of box_j (m, nparts + 1, 4)?  o_b = (w * h) / area_i[b] > overlap for any box b (max_b o_b >
    overlap: Matlab's max skips NaN, and a NaN o_b compares false)"""
    with np.errstate(all="ignore"):
        w = _vmin(box_i[None, :, 2], box_j[:, :, 2]) - _vmax(box_i[None, :, 0], box_j[:, :, 0]) + 1.0
        h = _vmin(box_i[None, :, 3], box_j[:, :, 3]) - _vmax(box_i[None, :, 1], box_j[:, :, 1]) + 1.0
        w = np.where(w < 0, 0.0, w)
        h = np.where(h < 0, 0.0, h)
        return (((w * h) / area_i[None, :]) > overlap).any(axis=1)


def nms_frame(rec: np.ndarray, nparts: int, overlap: float, max_boxes: int = MAX_BOXES) -> np.ndarray:
    """nms.m on one frame's records: the kept records in pick order"""
    overlap = float(np.float32(overlap))           # crosses the ABI as a float, widened in the comparison
    if len(rec) > max_boxes:
        rec = rec[score_order(scores(rec))[:max_boxes]]     # the list is REORDERED, as boxes(I(1:1000), :)
    box, area = nms_boxes(rec, nparts)
    order = np.array(pick_order(scores(rec)), np.int64)
    alive = np.ones(len(rec), bool)
    pick = []
    for i in order:
        if not alive[i]:
            continue
        pick.append(i)
        alive[order] &= ~covers(box[i], area[i], box[order], overlap)
        alive[i] = False                           # project decision: the pick itself always leaves
    return rec[pick]


def part_nms(rec: np.ndarray, nframes: int, nparts: int, overlap: float, max_boxes: int = MAX_BOXES,
             frame_offset: int = 0) -> np.ndarray:
    """pbd_part_nms: nms.m per frame of records grouped by ascending frame; frame by frame, the kept records in pick order"""
    rec = np.ascontiguousarray(rec, np.int32)
    fr = rec[:, 0].astype(np.int64) - frame_offset
    assert np.all(fr >= 0) and np.all(fr < nframes) and np.all(np.diff(fr) >= 0), "records grouped by ascending frame"
    out = [nms_frame(rec[fr == f], nparts, overlap, max_boxes) for f in range(nframes)]
    return np.concatenate(out, axis=0) if out else rec[:0]


def best_overlap(rec: np.ndarray, nframes: int, nparts: int, gtbox: np.ndarray, overlap: float, frame_offset: int = 0) -> tuple:
    """pbd_best_overlap: bestoverlap.m per frame.  gtbox (nframes, 4) float64 x1, y1, x2, y2 inclusive, a NaN anywhere in a
    row = no ground truth.  -> (nframes, stride) int32 (zeros where nothing is found), found (nframes,) int32"""
    rec = np.ascontiguousarray(rec, np.int32)
    gtbox = np.asarray(gtbox, np.float64).reshape(nframes, 4)
    overlap = float(np.float32(overlap))
    out = np.zeros((nframes, rec.shape[1]), np.int32)
    found = np.zeros(nframes, np.int32)
    s = scores(rec)
    c = centres(rec, nparts)
    best = [None] * nframes
    fr = rec[:, 0].astype(np.int64) - frame_offset
    with np.errstate(all="ignore"):
        for f in range(nframes):
            if np.isnan(gtbox[f]).any():
                continue
            idx = np.flatnonzero(fr == f)
            if not len(idx):
                continue
            x1, y1, x2, y2 = gtbox[f]
            area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
            bx1, bx2 = c[idx, :, 0].min(1), c[idx, :, 0].max(1)
            by1, by2 = c[idx, :, 1].min(1), c[idx, :, 1].max(1)
            w = _vmin(x2, bx2) - _vmax(x1, bx1) + 1.0
            h = _vmin(y2, by2) - _vmax(y1, by1) + 1.0
            w = np.where(w < 0, 0.0, w)
            h = np.where(h < 0, 0.0, h)
            ok = ((w * h) / area) > overlap
            for i in idx[ok]:
                if s[i] != s[i]:
                    continue                       # project decision: a NaN score is never chosen
                if best[f] is None or s[i] > s[best[f]]:       # ties: the first in list order (Matlab's max)
                    best[f] = i
    for f in range(nframes):
        if best[f] is not None:
            out[f] = rec[best[f]]
            found[f] = 1
    return out, found


def eval_pck(rec: np.ndarray, found: np.ndarray, nparts: int, gt_points: np.ndarray, scale: np.ndarray, thresh: float) -> tuple:
    """pbd_eval_pck: eval_pck.m on one record per frame (best_overlap's output).  gt_points (nframes, nparts, 2), scale
    (nframes,).  -> pck (nparts,), dist (nparts, nframes).  A frame that is not found has dist = +Inf; a NaN distance is the canonical quiet NaN and a miss.
    The reference's two quirks are NOT reproduced: its `nargin < 4` test always sets thresh = 0.5, and it uses the LAST
    frame's scale for every frame (a caller who wants that passes the last scale in every entry)."""
    rec = np.ascontiguousarray(rec, np.int32)
    nframes = len(rec)
    gt = np.asarray(gt_points, np.float64).reshape(nframes, nparts, 2)
    scale = np.asarray(scale, np.float64).reshape(nframes)
    c = centres(rec, nparts)
    dist = np.full((nparts, nframes), np.inf)
    pck = np.zeros(nparts)
    with np.errstate(all="ignore"):
        for p in range(nparts):
            hits = 0
            for f in range(nframes):
                if found[f]:
                    dx = c[f, p, 0] - gt[f, p, 0]
                    dy = c[f, p, 1] - gt[f, p, 1]
                    d = np.sqrt(np.float64(dx * dx) + np.float64(dy * dy))
                    dist[p, f] = d if d == d else np.nan       # one NaN (0x7ff8000000000000) for every source of it
                if dist[p, f] < np.float64(thresh) * scale[f]:
                    hits += 1
            pck[p] = np.float64(hits) / np.float64(nframes)
    return pck, dist


def voc_ap(rec: np.ndarray, prec: np.ndarray) -> float:
    """VOCap.m: the sum runs from 0.0 in ascending i, every product and addition rounded on its own"""
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = _max(mpre[i], mpre[i + 1])
    ap = np.float64(0.0)
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap = ap + np.float64((mrec[i] - mrec[i - 1]) * mpre[i])
    return float(ap)


def eval_apk(rec: np.ndarray, nframes: int, nparts: int, gt_offset: np.ndarray, gt_points: np.ndarray, gt_scale: np.ndarray,
             thresh: float, frame_offset: int = 0) -> tuple:
    """pbd_eval_apk: eval_apk.m + VOCap.m for every part at once.  Frame f's ground-truth instances are gt_offset[f] ..
    gt_offset[f + 1] - 1 of gt_points (G, nparts, 2) and gt_scale (G,).  -> apk (nparts,), prec, rec (nparts, n)"""
    rec_ = np.ascontiguousarray(rec, np.int32)
    n = len(rec_)
    gt_offset = np.asarray(gt_offset, np.int64)
    G = int(gt_offset[nframes])
    assert G > 0, "no ground truth: recall is 0 / 0"
    gt = np.asarray(gt_points, np.float64).reshape(G, nparts, 2)
    gs = np.asarray(gt_scale, np.float64).reshape(G)
    order = score_order(scores(rec_))
    c = centres(rec_, nparts)
    apk = np.zeros(nparts)
    prec = np.zeros((nparts, n))
    recall = np.zeros((nparts, n))
    fr = rec_[:, 0].astype(np.int64) - frame_offset
    jmin = np.full((n, nparts), -1, np.int64)
    distmin = np.zeros((n, nparts))
    with np.errstate(all="ignore"):
        for f in range(nframes):
            idx = np.flatnonzero(fr == f)
            for g in range(int(gt_offset[f]), int(gt_offset[f + 1])):
                dx = c[idx, :, 0] - gt[g, :, 0][None, :]
                dy = c[idx, :, 1] - gt[g, :, 1][None, :]
                d = np.sqrt(dx * dx + dy * dy) / gs[g]
                take = (d == d) & ((jmin[idx] < 0) | (d < distmin[idx]))       # NaN ignored; the FIRST minimum
                jmin[idx] = np.where(take, g, jmin[idx])
                distmin[idx] = np.where(take, d, distmin[idx])
        for p in range(nparts):
            det = np.zeros(G, bool)
            tpcum = 0
            for k, i in enumerate(order):
                j = jmin[i, p]
                if j >= 0 and distmin[i, p] <= thresh and not det[j]:
                    det[j] = True                  # gt(i).det(jmin)
                    tpcum += 1
                recall[p, k] = np.float64(tpcum) / np.float64(G)
                prec[p, k] = np.float64(tpcum) / np.float64(k + 1)    # every record is a true or a false positive
            apk[p] = voc_ap(recall[p], prec[p])
    return apk, prec, recall
