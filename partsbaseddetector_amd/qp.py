"""The training QP: the numpy yardstick of pbd_qp_* (include/pbd.h) and the QP class over the C ABI.

The problem is the one the reference's Matlab training code solves (matlab/learning/qp_write.m, qp_one.m with
oct/qp_one_sparse.cc, qp_opt.m, qp_refresh.m with oct/lincomb.cc, qp_prune.m, qp_w.m): a cache of block-sparse examples x'
(float32), their b and d, dual variables a in [0, 1] with sum <= 1 over a group of equal ids, and w = sum a x'.

``QPRef`` restates every call in the header's summation orders (``R``: 1024 lane-strided partial sums, then halving trees),
so that the device's results can be compared bit for bit.  ``QPRef(..., literal=True)`` uses sequential sums instead, as the
mex file adds; the CPU tests compare the two.  Nothing here runs on the GPU except the ``QP`` class.
"""
from __future__ import annotations

import ctypes as ct
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, synth
from .examples import strides, vector_offsets

LANES = 1024          # PBD_QP_LANES
_M64 = (1 << 64) - 1


# ---- summation orders ---------------------------------------------------------------------------------------------------
def reduce_r(p) -> float:
    """R(p): products p (float64, in value order) summed as include/pbd.h defines: lane l adds p[l], p[l + 1024], ... from
    +0.0; then per 64 lanes a halving tree (h = 32 .. 1); then a halving tree over the 16 sums (h = 8 .. 1)"""
    p = np.asarray(p, np.float64).ravel()
    m = max(1, -(-len(p) // LANES))
    P = np.zeros(m * LANES)
    P[:len(p)] = p
    P = P.reshape(m, LANES)
    acc = np.zeros(LANES)
    for r in range(m):
        acc = acc + P[r]
    s = acc.reshape(LANES // 64, 64).copy()
    h = 32
    while h >= 1:
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    t = s[:, 0].copy()
    h = LANES // 128
    while h >= 1:
        t[:h] = t[:h] + t[h:2 * h]
        h //= 2
    return float(t[0])


def reduce_seq(p) -> float:
    """sequential sum from 0.0 in value order (the mex file's score / dot loops)"""
    p = np.asarray(p, np.float64).ravel()
    if len(p) == 0:
        return 0.0
    return float(np.add.accumulate(np.concatenate([[0.0], p]))[-1])


def _div(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _min(a, b):   # MIN / MAX of qp_one_sparse.cc
    return b if a > b else a


def _max(a, b):
    return b if a < b else a


def seeded_order(seed: int, n: int) -> np.ndarray:
    """the pass order of pbd_qp_one without an explicit order: the stable argsort of synth.splitmix64(seed, n)"""
    return np.argsort(synth.splitmix64(int(seed) & _M64, n), kind="stable").astype(np.int32)


# ---- layout -------------------------------------------------------------------------------------------------------------
class Layout:
    """the model-vector layout of a flat model: its blocks, the example strides and model2vec's defaults"""

    def __init__(self, flat):
        dbase, fbase, n = vector_offsets(flat)
        self.L = n
        self.in_hw, self.V = strides(flat)
        self.MB = (self.in_hw - 4) // 2
        self.HW = 2 + 3 * self.MB
        self.blocks = [(b, 1) for b in range(dbase)] + [(dbase + 4 * d, 4) for d in range((fbase - dbase) // 4)]
        self.blocks += [(fbase + int(flat.filter_offset[f]), int(flat.filter_ksize[f]) ** 2 * flat.flen) for f in range(flat.nfilters)]
        self.slot_len = {}
        for off, ln in self.blocks:
            self.slot_len.setdefault(off, ln)
        self.wreg = np.ones(n)
        for c in range(flat.ncomponents):
            self.wreg[int(flat.biasid[flat.mix_offset[flat.part_offset[c]]])] = 0.01
        self.w0 = np.zeros(n)
        self.noneg = []
        for d in range((fbase - dbase) // 4):
            self.w0[dbase + 4 * d] = self.w0[dbase + 4 * d + 2] = 0.01
            self.noneg += [dbase + 4 * d, dbase + 4 * d + 2]
        self.noneg = np.asarray(self.noneg, np.int64)

    def header_ok(self, h) -> int:
        """-1: marked invalid; 0: not an example of this layout; 1: valid"""
        nb, nv = int(h[2]), int(h[3])
        if nb == -1:
            return -1
        if nb < 0 or nb > self.MB or nv < 0 or nv > self.V:
            return 0
        tot = 0
        for b in range(nb):
            off, ln = int(h[4 + 2 * b]), int(h[5 + 2 * b])
            if not 0 <= off < self.L or self.slot_len.get(off) != ln:
                return 0
            tot += ln
        return 1 if tot == nv else 0


class Entry:
    __slots__ = ("blocks", "x", "idx", "ids", "b", "d")

    def __init__(self, blocks, x, idx, ids, b, d):
        self.blocks, self.x, self.idx, self.ids, self.b, self.d = blocks, x, idx, ids, b, d

    def hdr(self, HW: int) -> np.ndarray:
        out = np.zeros(HW, np.int32)
        out[0], out[1] = len(self.blocks), len(self.x)
        for k, blk in enumerate(self.blocks):
            out[2 + 3 * k:5 + 3 * k] = blk
        return out


# ---- the yardstick ------------------------------------------------------------------------------------------------------
class QPRef:
    """pbd_qp_* in numpy.  flat: the model whose layout the examples follow; C, wpos, wreg, w0 and noneg as pbd_qp_config"""

    def __init__(self, flat, capacity: int, C: float = 0.002, wpos: float = 2.0, wreg=None, w0=None, noneg=None,
                 literal: bool = False):
        self.lay = Layout(flat)
        self.cap = int(capacity)
        self.Cpos, self.Cneg = float(C) * float(wpos), float(C)
        self.wreg = self.lay.wreg if wreg is None else np.asarray(wreg, np.float64)
        self.w0 = self.lay.w0 if w0 is None else np.asarray(w0, np.float64)
        self.noneg = self.lay.noneg if noneg is None else np.asarray(noneg, np.int64)
        self.R = reduce_seq if literal else reduce_r
        self.e: List[Entry] = []
        self.a: List[float] = []
        self.sv: List[int] = []
        self.nfix = 0
        self.w = np.zeros(self.lay.L)
        self.lb = self.ub = float("nan")
        self.loss = self.l = self.ww = 0.0
        self.have_lb = False
        self.lb_dropped = self.passes = self.converged = 0
        self.branches: List[str] = []     # per step of the last pass: "plain", "pair" or "none" (for the tests)
        self.detail: List[frozenset] = []  # per step of the last pass: the labels of _step that applied

    @property
    def n(self) -> int:
        return len(self.e)

    # -- qp_write
    def add(self, hdr, values, ids) -> int:
        """qp_write of examples in pbd_examples' format (hdr (n, hdr_words), values (n, values) of T); ids (n, 5).  The number
        written; invalid headers (nblocks -1) are skipped, others that do not follow the layout raise ValueError"""
        hdr = np.atleast_2d(np.asarray(hdr, np.int32))
        values = np.atleast_2d(np.asarray(values))
        ids = np.atleast_2d(np.asarray(ids, np.int32))
        for h in hdr:
            if self.lay.header_ok(h) == 0:
                raise ValueError("a header whose blocks are not blocks of the model vector")
        taken = 0
        for h, v, i in zip(hdr, values, ids):
            if self.lay.header_ok(h) != 1 or self.n >= self.cap:
                continue
            self._write(h, v, i)
            taken += 1
        return taken

    def _write(self, h, v, ids):
        label = int(ids[0]) > 0
        Cl = self.Cpos if label else self.Cneg
        inb, pos = [], 0
        for b in range(int(h[2])):
            off, ln = int(h[4 + 2 * b]), int(h[5 + 2 * b])
            inb.append((off, ln, pos))
            pos += ln
        blocks, xs, idxs, vneg = [], [], [], []
        ostart = 0
        done = set()
        for k, (off, ln, st) in enumerate(inb):
            if off in done:
                continue
            done.add(off)
            s = np.asarray(v[st:st + ln], np.float64)
            for off2, ln2, st2 in inb[k + 1:]:
                if off2 == off:
                    s = s + np.asarray(v[st2:st2 + ln2], np.float64)
            if not label:
                s = -s
            coords = np.arange(off, off + ln)
            xp = ((Cl * s) / self.wreg[coords]).astype(np.float32)
            blocks.append((off, ln, ostart))
            ostart += ln
            xs.append(xp)
            idxs.append(coords)
            vneg.append(s)
        x = np.concatenate(xs) if xs else np.zeros(0, np.float32)
        idx = np.concatenate(idxs) if idxs else np.zeros(0, np.int64)
        vn = np.concatenate(vneg) if vneg else np.zeros(0)
        b = Cl * (1.0 - self.R(self.w0[idx] * vn))
        x64 = x.astype(np.float64)
        d = self.R(x64 * x64)
        self.e.append(Entry(blocks, x, idx, tuple(int(t) for t in ids), b, d))
        self.a.append(0.0)
        self.sv.append(1)

    # -- train.m:75 (qp.n = 0) and detect.m:135 (the mining bound)
    def clear(self):
        """pbd_qp_clear: the state after create, except w (the next refresh rebuilds it)"""
        self.e, self.a, self.sv = [], [], []
        self.nfix = 0
        self.lb = self.ub = float("nan")
        self.loss = self.l = self.ww = 0.0
        self.have_lb = False
        self.lb_dropped = self.passes = self.converged = 0

    def _hinge(self, y: float, score: float) -> float:
        h = 1.0 - y * score
        return h if h > 0.0 else 0.0

    def _loss_records(self, records):
        """the records that count: every one present, written into the cache or dropped (detect.m:133-136)"""
        return records

    def add_loss(self, records, label: int) -> float:
        """pbd_qp_add_loss_device: ub += Cl * R(max(0, 1 - y * score_j)) over records (n, stride) int32 as a payload holds them
        (the float score in word 5); returns the addend"""
        if self.ub != self.ub:
            raise ValueError("no upper bound yet")
        r = np.asarray(records, np.int32)
        r = self._loss_records(r.reshape(len(r), -1) if r.size else np.zeros((0, 8), np.int32))
        scores = np.ascontiguousarray(r[:, 5]).view(np.float32).astype(np.float64)
        y = 1.0 if label > 0 else -1.0
        added = (self.Cpos if label > 0 else self.Cneg) * self.R(np.array([self._hinge(y, float(s)) for s in scores]))
        self.ub = self.ub + added
        return added

    def fix(self):
        self.nfix = self.n
        for i in range(self.n):
            self.sv[i] = 1

    # -- sums
    def wx(self, i: int, w=None) -> float:
        e = self.e[i]
        w = self.w if w is None else w
        return self.R(w[e.idx] * e.x.astype(np.float64))

    def xx(self, i: int, i2: int) -> float:
        e1, e2 = self.e[i], self.e[i2]
        pos2 = np.full(self.lay.L, -1, np.int64)
        pos2[e2.idx] = np.arange(len(e2.idx))
        p = pos2[e1.idx]
        x2 = e2.x.astype(np.float64)
        prod = np.where(p >= 0, e1.x.astype(np.float64) * x2[np.maximum(p, 0)] if len(x2) else 0.0, 0.0)
        return self.R(prod)

    def _axpy(self, da: float, i: int):
        e = self.e[i]
        self.w[e.idx] = self.w[e.idx] + da * e.x.astype(np.float64)

    def _clamp(self):
        """the non-negativity clamps; whether any coordinate changed"""
        v = self.w[self.noneg]
        self.w[self.noneg] = np.where(v < 0, 0.0, v)
        return bool(np.any(v < 0))

    def groups(self, members: Sequence[int]):
        """group numbers of members (ascending indices) by first appearance, and their count"""
        seen, g = {}, []
        for i in members:
            g.append(seen.setdefault(self.e[i].ids, len(seen)))
        return g, len(seen)

    # -- qp_refresh
    def _refresh_order(self):
        """the entries with a > 0 in ascending a, equal a by index: lincomb's order"""
        return sorted((i for i in range(self.n) if self.a[i] > 0), key=lambda i: (self.a[i], i))

    def refresh_tasks(self):
        """(offset, first coordinate, count) of the refresh's work items as the device forms them: every layout block that an
        entry with a > 0 carries, in pieces of at most 1024 coordinates.  A restatement of the host's split for the tests' own
        bookkeeping (which inputs make a block span two items); it is not compared with the device: what guards the split is the
        byte comparison of w"""
        used = {off for i in self._refresh_order() for off, ln, st in self.e[i].blocks}
        return [(off, c0, min(LANES, ln - c0)) for off, ln in sorted(self.lay.slot_len.items()) if off in used
                for c0 in range(0, ln, LANES)]

    def refresh(self):
        P = self._refresh_order()
        l = 0.0
        for i in P:
            l = l + self.e[i].b * self.a[i]
        self.w = np.zeros(self.lay.L)
        for i in P:
            self._axpy(self.a[i], i)
        self._clamp()
        self.ww = self.R(self.w * self.w)
        lb = l - self.ww * 0.5
        if self.have_lb and not lb > self.lb - 1e-5:
            self.lb_dropped = 1
        self.l, self.lb, self.have_lb = l, lb, True

    # -- qp_one
    def one(self, order=None, seed: int = 0):
        S = [i for i in range(self.n) if self.sv[i]]
        nsv = len(S)
        if nsv == 0:
            raise ValueError("no support vectors")
        perm = seeded_order(seed, nsv) if order is None else np.asarray(order, np.int64)
        if sorted(perm.tolist()) != list(range(nsv)):
            raise ValueError("order is not a permutation")
        gS, ng = self.groups(S)
        idC, idI, err = [0.0] * ng, [-1] * ng, [0.0] * ng
        for k, i in enumerate(S):
            idC[gS[k]] = idC[gS[k]] + self.a[i]
            if self.a[i] > 0:
                idI[gS[k]] = i
        self.branches, self.detail = [], []
        for k in perm:
            i, j = S[int(k)], gS[int(k)]
            self._step(i, j, idC, idI, err)
        loss = 0.0
        for v in err:
            loss = loss + v
        self.refresh()
        for i in range(self.nfix):
            self.sv[i] = 1
        self.loss = loss
        self.ub = self.ww * 0.5 + loss

    # -- one step of qp_one_sparse.cc.  Every comparison and every bound is one method, so that a test can restate a single rule
    # (tests/test_qp_hard_cpu.py); _step records in self.detail which of them applied.  The arithmetic and its order are the
    # mex file's.  Labels: plain_free / plain_floor0 / plain_cap_maxA; pair_up_free / pair_up_bound_1-Ai / pair_up_bound_A2 (dA > 0);
    # pair_down_free / pair_down_bound_-Ai / pair_down_bound_A2-1 (dA <= 0); pair_G_zeroed; pair_small_G; none_lower; none_upper;
    # i2_is_i; sv_clear; err_raised; G_is_0; clamp_changed_w_plain / _pair; pair_blocks_i2_lacks / _i2_extra / _shifted.  A bound's
    # label applies when the unbounded value reaches the bound and the result equals it: equal bounds give both labels.
    EPS = 1e-12

    def _is_lower(self, Ai, G):          # at the lower bound with a gradient that pushes further down
        return Ai == 0 and G >= 0

    def _is_upper(self, Ci, G):          # in a saturated group with a gradient that pushes further up
        return self._saturated(Ci) and G <= 0

    def _saturated(self, Ci):
        return Ci >= 1

    def _pair_saturated(self, Ci):       # the paired path's own "Ci >= 1"
        return self._saturated(Ci)

    def _clears_sv(self, Ai, G):         # strict: an entry at 0 with G == 0 stays a support vector
        return Ai == 0 and G > 0

    def _moves(self, G):
        return G > self.EPS or G < -self.EPS

    def _other(self, i2, i):
        return i2 != i

    def _pair_zeroes_G(self, Ai, G):
        return Ai == 0 and G > 0

    def _pair_zeroed_G(self, G):
        return 0.0

    def _plain_floor(self, x):
        return _max(x, 0.0)

    def _plain_cap(self, x, maxA):
        return _min(x, maxA)

    def _pair_up_own(self, dA, Ai):      # dA > 0: a[i] <= 1
        return _min(dA, 1.0 - Ai)

    def _pair_up_other(self, dA, A2):    # dA > 0: a[i2] >= 0
        return _min(dA, A2)

    def _pair_down_own(self, dA, Ai):    # dA <= 0: a[i] >= 0
        return _max(dA, -Ai)

    def _pair_down_other(self, dA, A2):  # dA <= 0: a[i2] <= 1
        return _max(dA, A2 - 1.0)

    def _plain_update(self, dA, i):
        self._axpy(dA, i)
        return self._clamp()

    def _pair_update(self, dA, i, i2):
        self._axpy(dA, i)
        self._axpy(-dA, i2)
        return self._clamp()

    def _note_err(self, err, j, G, det):
        if -G > err[j]:
            err[j] = -G
            det.add("err_raised")

    def _note_err_late(self, err, j, G, det):
        pass

    def _note_idI(self, idI, j, i):
        if self.a[i] > 0:
            idI[j] = i

    def _pair_blocks(self, i, i2, det):
        b1 = {off: st for off, ln, st in self.e[i].blocks}
        b2 = {off: st for off, ln, st in self.e[i2].blocks}
        if any(off not in b2 for off in b1):
            det.add("pair_blocks_i2_lacks")
        if any(off not in b1 for off in b2):
            det.add("pair_blocks_i2_extra")
        if any(off in b2 and b2[off] != st for off, st in b1.items()):
            det.add("pair_blocks_shifted")

    def _step(self, i, j, idC, idI, err):
        a = self.a
        det = set()
        Ai = _max(_min(a[i], 1.0), 0.0)
        a[i] = Ai
        Ci = _max(_min(idC[j], 1.0), Ai)
        G = self.wx(i) - self.e[i].b
        PG = G
        if G == 0:
            det.add("G_is_0")
        lower, upper = self._is_lower(Ai, G), self._is_upper(Ci, G)
        if lower or upper:
            PG = 0.0
        self._note_err(err, j, G, det)
        if self._clears_sv(Ai, G):
            self.sv[i] = 0
            det.add("sv_clear")
        i2 = idI[j]
        if i2 == i:
            det.add("i2_is_i")
        branch = "none"
        if self._pair_saturated(Ci) and G < -self.EPS and Ai < 1 and self._other(i2, i) and i2 >= 0:
            self._pair_blocks(i, i2, det)
            G = G - (self.wx(i2) - self.e[i2].b)
            if self._pair_zeroes_G(Ai, G):
                G = self._pair_zeroed_G(G)
                self.sv[i] = 0
                det.update(("pair_G_zeroed", "sv_clear"))
            if self._moves(G):
                A2 = a[i2]
                dA = _div(-G, self.e[i].d + self.e[i2].d - 2.0 * self.xx(i, i2))
                if dA > 0:
                    own, other = 1.0 - Ai, A2
                    raw, dA = dA, self._pair_up_other(self._pair_up_own(dA, Ai), A2)
                    hit = [n for n, b in (("pair_up_bound_1-Ai", own), ("pair_up_bound_A2", other)) if raw >= b and dA == b]
                    det.update(hit or ["pair_up_free"])
                else:
                    own, other = -Ai, A2 - 1.0
                    raw, dA = dA, self._pair_down_other(self._pair_down_own(dA, Ai), A2)
                    hit = [n for n, b in (("pair_down_bound_-Ai", own), ("pair_down_bound_A2-1", other)) if raw <= b and dA == b]
                    det.update(hit or ["pair_down_free"])
                a[i] = Ai + dA
                a[i2] = a[i2] - dA
                if self._pair_update(dA, i, i2):
                    det.add("clamp_changed_w_pair")
                branch = "pair"
            else:
                det.add("pair_small_G")
        elif self._moves(PG):
            maxA = 1.0 - (Ci - Ai)
            raw = Ai - _div(G, self.e[i].d)
            a[i] = self._plain_cap(self._plain_floor(raw), maxA)
            hit = [n for n, ok in (("plain_floor0", raw <= 0.0 and a[i] == 0.0), ("plain_cap_maxA", raw >= maxA and a[i] == maxA)) if ok]
            det.update(hit or ["plain_free"])
            dA = a[i] - Ai
            idC[j] = _min(_max(Ci + dA, 0.0), 1.0)
            if self._plain_update(dA, i):
                det.add("clamp_changed_w_plain")
            branch = "plain"
        else:
            if lower:
                det.add("none_lower")
            if upper:
                det.add("none_upper")
        self._note_err_late(err, j, G, det)
        self._note_idI(idI, j, i)
        self.branches.append(branch)
        self.detail.append(frozenset(det))

    # -- qp_opt
    def true_loss(self) -> float:
        g, ng = self.groups(range(self.n))
        best = [0.0] * ng
        for i in range(self.n):
            slack = -(self.wx(i) - self.e[i].b)
            if slack > best[g[i]]:
                best[g[i]] = slack
        s = 0.0
        for v in best:
            if v > 0:
                s = s + v
        return s

    def opt(self, tol: float = 0.05, iter: int = 1000, seed: int = 0, history: Optional[list] = None):
        if self.n == 0:
            raise ValueError("empty cache")
        self.lb_dropped = self.passes = self.converged = 0
        self.refresh()
        ub = self.ww * 0.5 + self.true_loss()
        self.sv = [1] * self.n
        for t in range(iter):
            self.one(seed=(seed + t) & _M64)
            self.passes = t + 1
            lb = self.lb
            ub_est = ub if ub < self.ub else self.ub
            if lb > 0 and 1 - lb / ub_est < tol:
                u = self.ww * 0.5 + self.true_loss()
                ub = u if u < ub else ub
                if 1 - lb / ub < tol:
                    self.converged = 1
                    if history is not None:
                        history.append(self.snapshot())
                    break
                self.sv = [1] * self.n
            if history is not None:
                history.append(self.snapshot())
        self.ub = ub

    # -- qp_prune
    def prune(self) -> int:
        self.lb_dropped = 0
        sv = list(self.sv)
        if all(sv):
            sv = [1 if (self.a[i] > 0 or i < self.nfix) else 0 for i in range(self.n)]
        keep = [i for i in range(self.n) if sv[i]]
        if not keep:
            raise ValueError("nothing to keep")
        self.nfix = sum(1 for i in keep if i < self.nfix)
        self.e = [self.e[i] for i in keep]
        self.a = [self.a[i] for i in keep]
        self.sv = [1] * len(keep)
        self.refresh()
        return self.n

    # -- qp_w, qp_scorepos
    def weights(self) -> np.ndarray:
        return self.w / self.wreg + self.w0

    def scores(self) -> np.ndarray:
        wraw = self.w + self.w0 * self.wreg
        return np.array([_div(self.wx(i, wraw), self.Cpos) for i in range(self.n) if self.e[i].ids[0] > 0])

    def snapshot(self) -> dict:
        return {"a": np.array(self.a), "sv": np.array(self.sv, np.uint8), "w": self.w.copy(), "lb": self.lb, "ub": self.ub,
                "loss": self.loss, "l": self.l, "n": self.n}

    def entries(self):
        """(hdr (n, HW) int32, values (n, V) float32, b, d, ids (n, 5)) as pbd_qp_entries returns them"""
        H = np.zeros((self.n, self.lay.HW), np.int32)
        X = np.zeros((self.n, self.lay.V), np.float32)
        for k, e in enumerate(self.e):
            H[k] = e.hdr(self.lay.HW)
            X[k, :len(e.x)] = e.x
        return (H, X, np.array([e.b for e in self.e]), np.array([e.d for e in self.e]),
                np.array([e.ids for e in self.e], np.int32).reshape(-1, 5))


def primal(flat_dense_x: np.ndarray, ids: Sequence[tuple], labels_C: np.ndarray, wreg, w0, v: np.ndarray) -> float:
    """the primal objective 1/2 |v|^2 + sum over groups of max(0, max_i C_i (1 - w . x_i)) with w = v / wreg + w0, from raw dense
    feature vectors (rows already negated for negatives): an independent certificate for weak duality"""
    w = v / wreg + w0
    margins = labels_C * (1.0 - flat_dense_x @ w)
    best = {}
    for m, i in zip(margins, ids):
        best[i] = max(best.get(i, 0.0), float(m))
    return 0.5 * float(v @ v) + sum(best.values())


def ids_of_records(records: np.ndarray, label: int, id_base: int = 0) -> np.ndarray:
    """detect.m's ex.id of records (n, stride): {label, id_base + frame, level, root x, root y}"""
    r = np.atleast_2d(np.asarray(records, np.int32))
    out = np.zeros((len(r), 5), np.int32)
    out[:, 0] = label
    out[:, 1] = id_base + r[:, 0]
    out[:, 2:5] = r[:, 2:5]
    return out


# ---- the device QP ------------------------------------------------------------------------------------------------------
class QP:
    """a pbd_qp: the training QP over a device-resident cache (include/pbd.h).  Created by PartsBasedDetector.qp(); outlives the
    detector.  Every method is synchronous."""

    def __init__(self, handle, capacity: int, C: float = 0.002, wpos: float = 2.0, wreg=None, w0=None, noneg=None, stream=None):
        self.lib = _lib.load()
        self._keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in
                      ((wreg, np.float64), (w0, np.float64), (noneg, np.int32))]
        wr, w0a, nn = self._keep
        cfg = _lib.CQpConfig(int(capacity), float(C), float(wpos), stream, None if wr is None else wr.ctypes.data,
                             None if w0a is None else w0a.ctypes.data, None if nn is None else nn.ctypes.data,
                             0 if nn is None else len(nn))
        q = ct.c_void_p()
        rc = self.lib.pbd_qp_create(handle.h, ct.byref(cfg), ct.byref(q))
        if rc != _lib.PBD_OK:
            raise _lib.PbdError(rc, self.lib.pbd_qp_last_error(None).decode())
        self.q = q
        info = self.state()
        self.len, self.hdr_words, self.values, self.capacity = info["len"], info["hdr_words"], info["values"], info["capacity"]

    def close(self):
        if getattr(self, "q", None):
            self.lib.pbd_qp_destroy(self.q)
            self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != _lib.PBD_OK:
            raise _lib.PbdError(rc, self.lib.pbd_qp_last_error(self.q).decode())
        return rc

    @staticmethod
    def _info(s: "_lib.CQpInfo") -> dict:
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "pad"}

    def add(self, handle, hdr, values, records=None, label: int = 1, id_base: int = 0, ids=None) -> int:
        """pbd_qp_add of host examples (pbd_examples' hdr / values of handle) with ids (n, 5), or the ids of their records"""
        hdr = np.ascontiguousarray(np.atleast_2d(hdr), np.int32)
        values = np.ascontiguousarray(np.atleast_2d(values), handle.dtype)
        ids = ids_of_records(records, label, id_base) if ids is None else np.ascontiguousarray(np.atleast_2d(ids), np.int32)
        n = len(hdr)
        if len(values) != n or len(ids) != n:
            raise _lib.PbdError(-1, "one values row and one id per header")
        t = ct.c_int()
        self.check(self.lib.pbd_qp_add(self.q, handle.h, n, hdr.ctypes.data if n else None, values.ctypes.data if n else None,
                                       ids.ctypes.data if n else None, ct.byref(t)))
        return t.value

    def add_device(self, handle, d_payload_ptr: int, capacity: int, d_hdr_ptr: int, d_values_ptr: int, label: int = 1,
                   id_base: int = 0, d_taken_ptr: Optional[int] = None) -> None:
        """pbd_qp_add_device of a pbd_examples_device call's outputs (device pointers)"""
        self.check(self.lib.pbd_qp_add_device(self.q, handle.h, d_payload_ptr, capacity, d_hdr_ptr, d_values_ptr, label, id_base,
                                              d_taken_ptr))

    def fix(self) -> None:
        self.check(self.lib.pbd_qp_fix(self.q))

    def clear(self) -> None:
        """pbd_qp_clear: an empty cache again (train.m:75), bounds NaN as after create"""
        self.check(self.lib.pbd_qp_clear(self.q))

    def add_loss_device(self, d_payload_ptr: int, capacity: int, label: int = -1) -> float:
        """pbd_qp_add_loss_device: ub += Cl * R(max(0, 1 - y * score)) over the records present in a device payload of the
        detector the QP was created from (detect.m:135); returns the addend"""
        added = ct.c_double()
        self.check(self.lib.pbd_qp_add_loss_device(self.q, d_payload_ptr, int(capacity), int(label), ct.byref(added)))
        return added.value

    def prune(self) -> int:
        n = ct.c_int()
        self.check(self.lib.pbd_qp_prune(self.q, ct.byref(n)))
        return n.value

    def one(self, order=None, seed: int = 0) -> dict:
        s = _lib.CQpInfo()
        o = None if order is None else np.ascontiguousarray(order, np.int32)
        self.check(self.lib.pbd_qp_one(self.q, None if o is None else o.ctypes.data, 0 if o is None else len(o), int(seed) & _M64,
                                       ct.byref(s)))
        return self._info(s)

    def opt(self, tol: float = 0.05, iter: int = 1000, seed: int = 0) -> dict:
        s = _lib.CQpInfo()
        self.check(self.lib.pbd_qp_opt(self.q, float(tol), int(iter), int(seed) & _M64, ct.byref(s)))
        return self._info(s)

    def weights(self) -> np.ndarray:
        """qp_w: the model vector (float64) for Model.from_vector"""
        w = np.zeros(self.len)
        self.check(self.lib.pbd_qp_weights(self.q, w.ctypes.data))
        return w

    def apply(self, handle) -> None:
        """pbd_qp_apply: the handle's parameters become weights() (rounded to its T), in place and on the device: afterwards the
        handle equals a new one created from Model.from_vector(weights())"""
        self.check(self.lib.pbd_qp_apply(self.q, handle.h))
        handle._model_stale = True

    def scores(self) -> np.ndarray:
        """qp_scorepos: the raw scores of the cached positives, ascending cache index"""
        s = np.zeros(max(self.capacity, 1))
        n = ct.c_int()
        self.check(self.lib.pbd_qp_scores(self.q, s.ctypes.data, ct.byref(n)))
        return s[:n.value].copy()

    def state(self, arrays: bool = False) -> dict:
        s = _lib.CQpInfo()
        self.check(self.lib.pbd_qp_state(self.q, ct.byref(s), None, None, None))
        out = self._info(s)
        if arrays:
            a = np.zeros(max(out["n"], 1))
            sv = np.zeros(max(out["n"], 1), np.uint8)
            w = np.zeros(out["len"])
            self.check(self.lib.pbd_qp_state(self.q, ct.byref(s), a.ctypes.data, sv.ctypes.data, w.ctypes.data))
            out.update(a=a[:out["n"]], sv=sv[:out["n"]], w=w)
        return out

    def entries(self, first: int = 0, count: Optional[int] = None):
        """(hdr (count, hdr_words) int32, values (count, values) float32, b, d, ids (count, 5)) of the cache entries"""
        n = self.state()["n"]
        count = n - first if count is None else count
        H = np.zeros((max(count, 1), self.hdr_words), np.int32)
        X = np.zeros((max(count, 1), self.values), np.float32)
        b, d = np.zeros(max(count, 1)), np.zeros(max(count, 1))
        ids = np.zeros((max(count, 1), 5), np.int32)
        self.check(self.lib.pbd_qp_entries(self.q, first, count, H.ctypes.data, X.ctypes.data, b.ctypes.data, d.ctypes.data,
                                           ids.ctypes.data))
        return H[:count], X[:count], b[:count], d[:count], ids[:count]
