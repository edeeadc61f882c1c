"""The max-marginals of every part and the poses they decode to, restated in numpy: the yardstick of pbd_max_marginals and
pbd_marginal_poses* (include/pbd.h).

The detector's root score answers "the best configuration rooted at this cell".  The max-marginal mm_p[m][y][x] answers the same
for every part: the best configuration with part p of type m at (x, y).  It is the upward pass's accumulated plane S_p[m] plus
what the rest of the tree contributes, ``down``, which a second, downward pass computes with the same generalised distance
transform, its quadratic mirrored (seen from the child) and its anchor negated.

Nothing here runs on the GPU: numpy plus ``oracle.dt`` (through examples.dt_raw), as examples.raw_maps and
partscores.accumulated are.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import examples as E
from . import partscores as PS


def reduce_max(values: Sequence[np.ndarray], first_wins: bool = True):
    """Math::reduceMax over a list of planes: strict > from -inf so that the first of equals wins, one plane copies.
    Returns (max, index).  first_wins False is the mutation (>=: the last of equals)."""
    if len(values) == 1:
        return np.array(values[0], copy=True), np.zeros(values[0].shape, np.int32)
    v = np.full(values[0].shape, -np.inf, values[0].dtype)
    best = np.zeros(values[0].shape, np.int32)
    with np.errstate(invalid="ignore"):
        for k, wv in enumerate(values):
            t = wv > v if first_wins else wv >= v
            best[t] = k
            v = np.where(t, wv, v)
    return v, best


def max_marginals(flat, c: int, resp: np.ndarray, *, sibling_order: str = "descending", skip_self: bool = True,
                  mirror_linear: bool = True, mirror_anchor: bool = True, first_wins: bool = True, readout: str = "reference",
                  nan_isect=None, contexts=None):
    """(mm, down, Jx, Jy, Jk) of component c on one level's responses resp (nfilters, H, W) of T.  mm and down are (NJ, H, W) of T,
    Jx / Jy / Jk (NJ, H, W) int32 with NJ the (part, type) pairs of the MODEL; planes of other components stay 0 (values) and the
    root's pointer planes are -1.

    readout names the read-out rule of every transform, upward and mirrored ("reference" or "max", as oracle.dt takes it).  On
    finite inputs the two agree; for inputs with +-Inf or NaN the yardstick of pbd_max_marginals is the rule run with "max", the
    library's decision where a NaN intersection forms (include/pbd.h, pbd_dp_min, "Non-finite scores", item 3).  nan_isect, a
    dict, receives the NaN intersections the oracle counted: "upward" over the transforms D_p[m], "mirrored" over R_p[m][mq];
    contexts, a dict, receives the context planes C_p[mq] under the key (p, mq), the inputs of the mirrored transforms.

    The keyword arguments are NOT part of the rule: each names one choice the rule makes (the siblings' messages added in descending
    index order, a part's own message left out of its context, the linear coefficients negated, the anchor negated, the first of
    equal parent types wins) and its other value is the mutation tests/test_marginals_cpu.py shows to change an output."""
    from oracle import oracle
    T = resp.dtype.type
    _, H, W = resp.shape
    p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
    n = p1 - p0
    NJ = int(flat.mix_offset[-1])
    mm = np.zeros((NJ, H, W), resp.dtype)
    down = np.zeros((NJ, H, W), resp.dtype)
    Jx = np.zeros((NJ, H, W), np.int32)
    Jy = np.zeros((NJ, H, W), np.int32)
    Jk = np.zeros((NJ, H, W), np.int32)
    planes = PS.accumulated(flat, c, resp, readout=readout)[5]        # S_p[m]
    n_up, n_mir = [0], [0]
    gms = lambda p: range(int(flat.mix_offset[p0 + p]), int(flat.mix_offset[p0 + p + 1]))
    parent = [int(flat.parentid[p0 + p]) for p in range(n)]
    children = [[q for q in range(n - 1, 0, -1) if parent[q] == p] for p in range(n)]      # descending index
    bias = lambda gm, mq: T(np.float32(flat.biasw[int(flat.biasid[gm]) + mq]))

    # the upward messages M_p[mq], from the transforms of the accumulated planes
    M = {}
    for p in range(1, n):
        D = []
        for m, gm in enumerate(gms(p)):
            d = int(flat.defid[gm])
            w = [float(v) for v in flat.defw[d]]
            D.append(E.dt_raw(oracle, np.ascontiguousarray(planes[p][m]), -w[0], -w[1], -w[2], -w[3], int(flat.anchors[d][0]),
                              int(flat.anchors[d][1]), readout=readout, nan_isect=n_up)[0])
        for mq in range(len(gms(parent[p]))):
            M[p, mq] = reduce_max([D[m] + bias(gm, mq) for m, gm in enumerate(gms(p))])[0]

    depth = [0] * n
    for p in range(1, n):
        depth[p] = depth[parent[p]] + 1
    g0 = int(flat.mix_offset[p0])
    for m, gm in enumerate(gms(0)):
        down[gm] = T(np.float32(flat.biasw[int(flat.biasid[g0])]))       # the root bias of type 0, for every root type
        mm[gm] = planes[0][m] + down[gm]
        Jx[gm] = Jy[gm] = Jk[gm] = -1
    cols = np.arange(W)[None, :]
    for p in sorted(range(1, n), key=lambda q: (depth[q], q)):
        q = parent[p]
        ctx = []
        for mq, gq in enumerate(gms(q)):
            C = np.array(resp[int(flat.filterid[gq])], copy=True)
            sibs = children[q] if sibling_order == "descending" else children[q][::-1]
            for s in sibs:
                if s == p and skip_self:
                    continue
                C = C + M[s, mq]
            ctx.append(C + down[gq])
            if contexts is not None:
                contexts[p, mq] = ctx[-1]
        for m, gm in enumerate(gms(p)):
            d = int(flat.defid[gm])
            w = [float(v) for v in flat.defw[d]]
            ox, oy = int(flat.anchors[d][0]), int(flat.anchors[d][1])
            sl = -1.0 if mirror_linear else 1.0
            sa = -1 if mirror_anchor else 1
            R, px, py = [], [], []
            for mq in range(len(ctx)):
                o, ix, iy = E.dt_raw(oracle, np.ascontiguousarray(ctx[mq]), -w[0], sl * -w[1], -w[2], sl * -w[3], sa * ox, sa * oy,
                                     readout=readout, nan_isect=n_mir)
                R.append(o + bias(gm, mq))
                py.append(iy)                                  # the columns pass's pointer first,
                px.append(ix[iy, cols])                        # then the rows pass's at that row
            down[gm], Jk[gm] = reduce_max(R, first_wins)
            Jx[gm] = np.take_along_axis(np.stack(px), Jk[gm][None], 0)[0]
            Jy[gm] = np.take_along_axis(np.stack(py), Jk[gm][None], 0)[0]
            mm[gm] = planes[p][m] + down[gm]
    if nan_isect is not None:
        nan_isect["upward"] = nan_isect.get("upward", 0) + n_up[0]
        nan_isect["mirrored"] = nan_isect.get("mirrored", 0) + n_mir[0]
    return mm, down, Jx, Jy, Jk


def decode(flat, c: int, level: int, part: int, mtype: int, x: int, y: int, mm, Jx, Jy, Jk, IxRaw, IyRaw, Ik, scale, frame: int = 0,
           frame_offset: int = 0, dtype=np.float32) -> Tuple[List[Tuple[int, int, int]], np.ndarray]:
    """(placement [(x, y, type)] of every part, record int32[stride]) of the seed (level, c, part, mtype or -1, x, y): the climb
    through Jk / Jx / Jy to the root fixes the parts on that path; every other part, in index order, takes examples.walk's arg-max
    step from its parent's placement on the upward maps IxRaw / IyRaw / Ik of examples.raw_maps.  Type -1 is reduce_max's choice:
    type 0 where no mm is above -inf (every one NaN or -inf); the score is the mm of the type decoded."""
    p0 = int(flat.part_offset[c])
    n = int(flat.part_offset[c + 1]) - p0
    g = lambda p: int(flat.mix_offset[p0 + p])
    K = int(flat.mix_offset[p0 + part + 1]) - g(part)
    if mtype < 0:
        vals = [mm[g(part) + t, y, x] for t in range(K)]
        mtype = 0
        if K > 1:
            best = -np.inf
            for t, v in enumerate(vals):
                if v > best:
                    best, mtype = v, t
    score = np.float32(mm[g(part) + mtype, y, x])
    place = [None] * n
    q, cx, cy, t = part, x, y, mtype
    while True:
        place[q] = (cx, cy, t)
        if q == 0:
            break
        gm = g(q) + t
        cx, cy, t = int(Jx[gm, cy, cx]), int(Jy[gm, cy, cx]), int(Jk[gm, cy, cx])
        q = int(flat.parentid[p0 + q])
    for q in range(1, n):
        if place[q] is not None:
            continue
        px, py, pm = place[int(flat.parentid[p0 + q])]
        s = int(flat.ptr_slot[p0 + q]) + pm
        m = int(Ik[s, py, px])
        k = g(q) + m
        ny = int(IyRaw[k, py, px])
        place[q] = (int(IxRaw[k, ny, px]), ny, m)
    rec = np.zeros(8 + 4 * int(flat.max_parts), np.int32)
    rec[0], rec[1], rec[2] = frame + frame_offset, c, level
    rec[3], rec[4] = place[0][0], place[0][1]
    rec[5] = np.array([score], np.float32).view(np.int32)[0]
    rec[6], rec[7] = n, place[0][2]
    for q, (qx, qy, qm) in enumerate(place):
        ks = int(flat.filter_ksize[int(flat.filterid[g(q) + qm])])
        x1, y1, x2, y2 = E.part_rects(qx, qy, ks, scale, dtype)
        rec[8 + 4 * q: 12 + 4 * q] = [x1, y1, x2 - x1, y2 - y1]
    return place, rec


def seed_valid(flat, shapes, seed) -> bool:
    """a seed pbd_marginal_poses accepts: level, component, part and type in range (type -1 allowed), the cell inside the map"""
    l, c, p, m, x, y = (int(v) for v in seed)
    if not (0 <= l < len(shapes) and 0 <= c < flat.ncomponents):
        return False
    p0 = int(flat.part_offset[c])
    if not 0 <= p < int(flat.part_offset[c + 1]) - p0:
        return False
    H, W = shapes[l]
    return -1 <= m < int(flat.mix_offset[p0 + p + 1]) - int(flat.mix_offset[p0 + p]) and 0 <= x < W and 0 <= y < H
