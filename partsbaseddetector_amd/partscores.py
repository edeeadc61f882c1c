"""The score of each part of a detection, restated in numpy: the yardstick of pbd_part_scores* and pbd_score_placements*
(include/pbd.h).

A detection's score is a sum the dynamic program builds bottom-up: every part's filter response at its cell, plus for every
child the bias and the (negative) deformation cost of its displacement from its parent.  ``part_scores`` takes that sum apart
again at a placement, with the roundings of the dynamic program itself: per part {appearance, message, bias, total}.

Nothing here runs on the GPU.  ``accumulated`` restates DynamicProgram::min as examples.raw_maps does and also returns the plane
every part had accumulated when its parent consumed it, which is what ``total`` is compared with.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import examples as E

APPEARANCE, MESSAGE, BIAS, TOTAL = 0, 1, 2, 3


def quad_val(a: float, b: float, d: int, y, T):
    """Quadratic::operator()(x, y) (include/DistanceTransform.hpp:102-104): the int square, double arithmetic left to right, one
    rounding to T"""
    return T(a * float(d * d) + b * float(d) + float(y))


def part_scores(flat, resp: np.ndarray, c: int, placement, dtype=np.float32, *, child_order: str = "descending",
                passes: str = "two", root_bias: str = "mixture0") -> np.ndarray:
    """(nparts, 4) of T: appearance, message, bias, total of every part of component c at placement [(x, y, m)] on one level's
    resident responses resp (nfilters, H, W).

    The keyword arguments are NOT part of the rule: each names one choice the rule makes (the reference's descending child order,
    one rounding per pass of the transform, the root's bias of mixture 0) and its other value is the mutation
    tests/test_partscores_cpu.py shows to change a value."""
    T = np.dtype(dtype).type
    p0 = int(flat.part_offset[c])
    n = int(flat.part_offset[c + 1]) - p0
    app, bias, msg = [T(0)] * n, [T(0)] * n, [T(0)] * n
    for p, (x, y, m) in enumerate(placement):
        gm = int(flat.mix_offset[p0 + p]) + m
        app[p] = T(resp[int(flat.filterid[gm]), y, x])
        if p == 0:
            g0 = int(flat.mix_offset[p0]) + (m if root_bias == "winning" else 0)
            bias[p] = T(np.float32(flat.biasw[int(flat.biasid[g0])]))
        else:
            pm = placement[int(flat.parentid[p0 + p])][2]
            bias[p] = T(np.float32(flat.biasw[int(flat.biasid[gm]) + pm]))
    total = list(app)
    order = range(n - 1, 0, -1) if child_order == "descending" else range(1, n)
    if child_order != "descending":
        # ascending order needs every child's total complete before it is consumed: deepest parts first, ascending among siblings
        depth = [0] * n
        for q in range(1, n):
            depth[q] = depth[int(flat.parentid[p0 + q])] + 1
        order = sorted(range(1, n), key=lambda q: (-depth[q], q))
    for q in order:
        x, y, m = placement[q]
        par = int(flat.parentid[p0 + q])
        px, py, _ = placement[par]
        d = int(flat.defid[int(flat.mix_offset[p0 + q]) + m])
        w = [float(np.float32(v)) for v in flat.defw[d]]
        dx, dy = px + int(flat.anchors[d][0]) - x, py + int(flat.anchors[d][1]) - y
        if passes == "two":
            r = quad_val(-w[0], -w[1], dx, total[q], T)
            msg[q] = quad_val(-w[2], -w[3], dy, r, T)
        else:
            msg[q] = T(-w[2] * float(dy * dy) + -w[3] * float(dy) + (-w[0] * float(dx * dx) + -w[1] * float(dx) + float(total[q])))
        total[par] = T(total[par] + T(msg[q] + bias[q]))
    msg[0] = T(total[0] + bias[0])
    return np.array([[app[p], msg[p], bias[p], total[p]] for p in range(n)], dtype)


def accumulated(flat, c: int, resp: np.ndarray, readout: str = "reference"):
    """DynamicProgram::min of component c on one level's responses, as examples.raw_maps restates it, which also keeps what
    raw_maps drops: returns (IxRaw, IyRaw, Ik, rootv, rooti, planes) with planes[p][m] the (H, W) plane part p's mixture m had
    accumulated when it was consumed (a child: when its transform ran; the root: when the root scores were taken).  The planes
    are kept per filter id as the reference keeps them, so parts that share an inner filter id see each other's messages.
    readout: the transform's read-out rule, as examples.dt_raw takes it."""
    from oracle import oracle
    T = resp.dtype.type
    _, H, W = resp.shape
    p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
    totmix = int(flat.mix_offset[-1])
    IxRaw = np.zeros((totmix, H, W), np.int32)
    IyRaw = np.zeros((totmix, H, W), np.int32)
    Ik = np.zeros((max(flat.nslots, 1), H, W), np.int32)
    nc, planes = {}, {}
    for gp in range(p1 - 1, p0, -1):
        g0, g1 = int(flat.mix_offset[gp]), int(flat.mix_offset[gp + 1])
        gpar = p0 + int(flat.parentid[gp])
        sc, planes[gp - p0] = [], []
        for gm in range(g0, g1):
            f, d = int(flat.filterid[gm]), int(flat.defid[gm])
            w = [float(v) for v in flat.defw[d]]
            src = np.ascontiguousarray(nc.get(f, resp[f]))
            planes[gp - p0].append(np.array(src, copy=True))
            o, IxRaw[gm], IyRaw[gm] = E.dt_raw(oracle, src, -w[0], -w[1], -w[2], -w[3], int(flat.anchors[d][0]),
                                               int(flat.anchors[d][1]), readout=readout)
            sc.append(o)
        for pm in range(int(flat.mix_offset[gpar + 1]) - int(flat.mix_offset[gpar])):
            fp = int(flat.filterid[int(flat.mix_offset[gpar]) + pm])
            if fp not in nc:
                nc[fp] = np.array(resp[fp], copy=True)
            v = np.full((H, W), -np.inf, resp.dtype)
            best = np.zeros((H, W), np.int32)
            if g1 - g0 == 1:
                v = sc[0] + T(flat.biasw[int(flat.biasid[g0]) + pm])
            else:
                for mm in range(g1 - g0):
                    wv = sc[mm] + T(flat.biasw[int(flat.biasid[g0 + mm]) + pm])
                    t = wv > v
                    best[t] = mm
                    v = np.where(t, wv, v)
            Ik[int(flat.ptr_slot[gp]) + pm] = best
            nc[fp] = nc[fp] + v
    g0, g1 = int(flat.mix_offset[p0]), int(flat.mix_offset[p0 + 1])
    bias = T(flat.biasw[int(flat.biasid[g0])])
    planes[0] = [np.array(nc.get(int(flat.filterid[gm]), resp[int(flat.filterid[gm])]), copy=True) for gm in range(g0, g1)]
    if g1 - g0 == 1:
        rootv, rooti = planes[0][0] + bias, np.zeros((H, W), np.int32)
    else:
        rootv, rooti = np.full((H, W), -np.inf, resp.dtype), np.zeros((H, W), np.int32)
        for mm in range(g1 - g0):
            wv = planes[0][mm] + bias
            t = wv > rootv
            rooti[t] = mm
            rootv = np.where(t, wv, rootv)
    return IxRaw, IyRaw, Ik, rootv.astype(resp.dtype), rooti, planes


def placement_valid(flat, c: int, placement, H: int, W: int) -> bool:
    """every cell inside the H x W map and every mixture one of its part's (pbd_score_placements' status)"""
    p0 = int(flat.part_offset[c])
    for p, (x, y, m) in enumerate(placement):
        if not (0 <= x < W and 0 <= y < H and 0 <= m < int(flat.mix_offset[p0 + p + 1]) - int(flat.mix_offset[p0 + p])):
            return False
    return True


def scores_of_records(flat, frames: Sequence["E.FrameMaps"], records: np.ndarray, frame_offset: int = 0, dtype=np.float32,
                      walk: str = None, place: np.ndarray = None, resp_of=None, fill=0):
    """(status (n,), place (n, max_parts, 3), scores (n, max_parts, 4)) of records (n, stride) int32 as pbd_part_scores returns
    them (entries past a record's parts keep ``fill``); frames[f] holds the oracle's maps of frame f and walk "reference" /
    "argmax" names the walk (None: each frame's own).  place given: pbd_score_placements -- those placements instead of the
    walk's, status -1 and nothing else for one outside the map or its part's mixtures.  resp_of(frame, level) replaces the
    oracle's responses by the caller's (the resident ones of an inexact convolution mode, read back)."""
    records = np.atleast_2d(np.asarray(records, np.int32))
    n, mp = len(records), int(flat.max_parts)
    status = np.full(n, fill, np.int32)
    out_place = np.full((n, mp, 3), fill, np.int32)
    scores = np.full((n, mp, 4), fill, dtype)
    for i, r in enumerate(records):
        f, c, lvl = int(r[0]) - frame_offset, int(r[1]), int(r[2])
        fm = frames[f]
        resp = fm.resp(lvl) if resp_of is None else resp_of(f, lvl)
        k = int(flat.part_offset[c + 1]) - int(flat.part_offset[c])
        if place is None:
            pl = fm.placement(lvl, c, int(r[3]), int(r[4]), walk)
        else:
            pl = [tuple(int(v) for v in q) for q in place[i, :k]]
            if not placement_valid(flat, c, pl, resp.shape[1], resp.shape[2]):
                status[i] = -1
                continue
        status[i] = k
        out_place[i, :k] = np.asarray(pl, np.int32)
        scores[i, :k] = part_scores(flat, resp, c, pl, dtype)
    return status, out_place, scores
