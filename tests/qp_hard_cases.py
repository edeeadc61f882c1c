"""Examples that drive the training QP -- k_qp_slots, k_qp_write, k_qp_score, k_qp_pass, k_qp_lincomb, k_qp_norm and k_qp_gather
in pbd_kernels_qp.hip -- into what mined examples never reach: entries of 1 to nearly V values with and without a bias block,
blocks whose first output value lies past 1024 and off the lane grid, offsets used two and three times, headers marked
invalid on wave and workgroup boundaries, id groups of 1, 3, 4 and 5, and every outcome of a step of qp_one_sparse (which bound
wins each clamp, exact zeros of the gradient, groups that reach 1.0 exactly, paired updates whose two bounds tie).

numpy only and no handle: each set is hdr / values / ids in pbd_examples' format for the layout of a model, with the QP's
configuration and the pass orders.  Shared by tests/test_qp_hard_cpu.py (QPRef alone: what the sets reach, and that a changed
rule changes the result) and tests/test_gpu_qp_hard.py (the kernels against QPRef, byte for byte)."""
import itertools

import numpy as np

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd import synth

C_GRID = 2.0 ** -9          # the exact cases: C, and values that are single powers of two


def mixed_model():
    """4 parts x 3 mixtures with 5x5, 3x3, 7x7 and 4x4 filters: blocks of 1 / 4 / 288 / 512 / 800 / 1568 values, V = 5520, MB = 11"""
    return M.synthetic_model(seed=17, pa=[0, 1, 1, 2], nmix=3, ksize=[5, 3, 7, 4], interval=5, name="qp_mixed")


def tiny_model():
    return M.synthetic_tiny_model()


MODELS = {"mixed": mixed_model, "tiny": tiny_model}


class Blocks:
    """the layout's blocks by kind: B.bias[k], B.defs[k], B.filt[length][k] are (offset, length)"""

    def __init__(self, flat):
        self.lay = Q.Layout(flat)
        self.dbase, self.fbase, self.L = E.vector_offsets(flat)
        blocks = sorted(self.lay.slot_len.items())
        self.bias = [b for b in blocks if b[0] < self.dbase]
        self.defs = [b for b in blocks if self.dbase <= b[0] < self.fbase]
        self.filt = {}
        for b in blocks:
            if b[0] >= self.fbase:
                self.filt.setdefault(b[1], []).append(b)


class Set:
    """one set of examples with the QP configuration it is meant for"""

    def __init__(self, name, model, hdr, values, ids, passes=5, seed=0, **cfg):
        self.name, self.model, self.hdr, self.values, self.ids = name, model, hdr, values, np.asarray(ids, np.int32)
        self.passes, self.seed, self.cfg = passes, seed, cfg
        self.orders = None       # explicit orders (one list per pass), or seeded permutations of the support vectors
        self.tie_sensitive = False

    def ref(self, cls=Q.QPRef, capacity=None, **kw):
        flat = MODELS[self.model]().flatten()
        cfg = dict(self.cfg)
        cfg.update(kw)
        return cls(flat, capacity or len(self.hdr) + 8, **cfg)

    def order(self, t, sv):
        """pass t's order over the support vectors (sv: the cache's flags): the explicit order of entries, as their ranks among
        the support vectors (an entry that is none is left out), or a seeded permutation"""
        sv = np.asarray(sv)
        if self.orders is not None:
            rank = np.cumsum(sv != 0) - 1
            return np.asarray([rank[i] for i in self.orders[t] if sv[i]], np.int32)
        return np.random.RandomState(1000 * self.seed + t).permutation(int(np.sum(sv != 0))).astype(np.int32)


def pack(lay, examples, dtype=np.float64):
    """examples: lists of ((offset, length), values) -> hdr (n, in_hw) int32 and values (n, V) of dtype"""
    hdr = np.zeros((len(examples), lay.in_hw), np.int32)
    vals = np.zeros((len(examples), lay.V), dtype)
    for i, ex in enumerate(examples):
        v = np.concatenate([np.asarray(x, np.float64).ravel() for _, x in ex]) if ex else np.zeros(0)
        assert len(ex) <= lay.MB and len(v) <= lay.V and all(len(np.ravel(x)) == b[1] for b, x in ex)
        hdr[i, :4] = (i, 0, len(ex), len(v))
        hdr[i, 4:4 + 2 * len(ex)] = np.asarray([b for b, _ in ex], np.int32).ravel()
        vals[i, :len(v)] = v
    return hdr, vals


def invalid_header(lay, i):
    h = np.zeros(lay.in_hw, np.int32)
    h[:4] = (i, 0, -1, 0)
    return h


def block_values(block, seed, scale):
    """seeded raw feature values of a block, as a detector's examples hold them: 1 for a bias, -(dx^2, dx, dy^2, dy), HOG-like
    values for a filter"""
    off, ln = block
    if ln == 1:
        return np.ones(1)
    if ln == 4:
        dx, dy = synth.randint(seed, 2, -3, 3, stream=off)
        return np.array([-(dx * dx), -dx, -(dy * dy), -dy], np.float64)
    return scale * 0.25 * synth.normalish(seed * 7919 + 13, ln, stream=off)


def ids_in_groups(n, npos, sizes=(1, 3, 4, 5), base=100):
    """positives one id each; negatives in id groups whose sizes cycle through `sizes`"""
    ids = np.zeros((n, 5), np.int32)
    ids[:npos, 0] = 1
    ids[:npos, 1] = np.arange(npos)
    ids[npos:, 0] = -1
    g, left = 0, 0
    for i in range(npos, n):
        if left == 0:
            g += 1
            left = sizes[(g - 1) % len(sizes)]
        ids[i, 1] = base + g
        ids[i, 2] = g % 7          # the whole id row is the group's key
        left -= 1
    return ids


# ---- shapes -------------------------------------------------------------------------------------------------------------
def nearest_nv(B, target):
    """the entry sizes nearest to target that distinct blocks of the layout (at most MB of them) can form"""
    kinds = [(1, len(B.bias)), (4, len(B.defs))] + [(ln, len(v)) for ln, v in sorted(B.filt.items())]
    best = None
    for counts in itertools.product(*[range(min(c, B.lay.MB) + 1) for _, c in kinds]):
        if 0 < sum(counts) <= B.lay.MB:
            nv = sum(c * ln for c, (ln, _) in zip(counts, kinds))
            if nv <= B.lay.V and (best is None or abs(nv - target) < abs(best - target)):
                best = nv
    return best


def shape_list(B):
    """the explicit shapes of the mixed model: (name, blocks).  nv = 1, 4, 5, 16, 288, 1024 (two 4x4 filters, no bias), 1025, 1573,
    2080 (the nearest to 2048 this layout forms; its second block starts at output value 1568: past 1024, off the lane grid),
    5519 (11 = MB blocks, one value short of V) and ordinary mixtures of them"""
    f = B.filt
    return [
        ("nv1", [B.bias[1]]),
        ("nv4", [B.defs[0]]),
        ("nv5", [B.bias[2], B.defs[1]]),
        ("nv16", [B.bias[0], B.bias[1], B.bias[2], B.bias[3], B.defs[0], B.defs[1], B.defs[2]]),
        ("nv288", [f[288][0]]),
        ("nv1024", [f[512][0], f[512][1]]),
        ("nv1025", [B.bias[0], f[512][0], f[512][1]]),
        ("nv1573", [B.bias[0], B.defs[0], f[1568][0]]),
        ("nv2080", [f[1568][0], f[512][0]]),
        ("nv5519", [B.bias[0], B.bias[4], B.bias[5], B.defs[0], B.defs[3], B.defs[4], f[1568][0], f[1568][1], f[1568][2], f[512][2],
                    f[288][1]]),
        ("root", [B.bias[0], f[800][0]]),
        ("two", [B.bias[0], B.bias[4], B.defs[0], f[800][0], f[288][0]]),
        ("two_b", [B.bias[0], B.bias[5], B.defs[1], f[800][0], f[288][1]]),
        ("three", [B.bias[0], B.bias[4], B.bias[7], B.defs[0], B.defs[3], f[800][0], f[288][0], f[1568][0]]),
        ("shift", [B.bias[0], f[288][0], f[800][0]]),          # the blocks of "root" and "two" at other positions
        ("full", [B.bias[0], B.bias[4], B.bias[7], B.bias[10], B.defs[0], B.defs[3], B.defs[6], f[800][0], f[288][0], f[1568][0],
                  f[512][0]]),
    ]


def shape_set(name="shapes", copies=5, npos=12, scale=1.0, seed=1, dtype=np.float64, **cfg):
    """`copies` seeded examples of every shape of shape_list on the mixed model, shuffled; the first npos are positives with one
    id each, the rest negatives in id groups of 1, 3, 4 and 5"""
    B = Blocks(mixed_model().flatten())
    shapes = shape_list(B)
    ex = []
    for c in range(copies):
        for k, (_, blocks) in enumerate(shapes):
            ex.append([(b, block_values(b, 97 * c + k + seed, scale)) for b in blocks])
    perm = np.random.RandomState(seed).permutation(len(ex))
    ex = [ex[i] for i in perm]
    hdr, vals = pack(B.lay, ex, dtype)
    s = Set(name, "mixed", hdr, vals, ids_in_groups(len(ex), npos), seed=seed, **cfg)
    s.tie_sensitive = True      # groups saturate: "Ci >= 1" is an exact compare
    return s


def one_id_set(name="one_id", n=40, npos=15, seed=11, tripled=16):
    """full-scale examples of the tiny model with one id each: Ci >= 1 only by one entry's own a.  The last `tripled` examples
    are the first ones' values times 3 under ids of their own: whichever of the two is stepped first takes a > 0, the other
    then overshoots the margin they share, and the first one's next plain step is floored at 0"""
    flat = tiny_model().flatten()
    B = Blocks(flat)
    f = B.filt[800]
    r = synth.randint(seed, 8 * n, 0, 1 << 20, stream=3)
    ex = []
    for i in range(n):
        blocks = [B.bias[int(r[8 * i] % len(B.bias))]]
        for k in range(2):
            d = B.defs[int(r[8 * i + 1 + k] % len(B.defs))]
            if d not in blocks:
                blocks.append(d)
        for fi in sorted({int(r[8 * i + 3 + k] % len(f)) for k in range(2)}):
            blocks.append(f[fi])
        ex.append([(b, block_values(b, seed + i, 1.0)) for b in blocks])
    src = [npos - tripled // 2 + k for k in range(tripled)]      # positives and negatives
    ex += [[(b, 3.0 * v) for b, v in ex[i]] for i in src]
    hdr, vals = pack(B.lay, ex)
    ids = np.zeros((len(ex), 5), np.int32)
    ids[:, 0] = np.where(np.arange(len(ex)) < npos, 1, -1)
    ids[n:, 0] = ids[src, 0]
    ids[:, 1] = np.arange(len(ex))
    return Set(name, "tiny", hdr, vals, ids, passes=6, seed=seed)


# ---- duplicate offsets --------------------------------------------------------------------------------------------------
def dup_set(dtype=np.float64):
    """offsets used more than once (k_qp_write's lead / nxt chains): A A A B (three times, as the first block), bias A B A,
    A B A B A, a deformation block twice around a bias, a bias twice as the first block; with plain copies to pair with"""
    B = Blocks(mixed_model().flatten())
    A, Bk, Cc = B.filt[288][0], B.filt[512][0], B.filt[1568][0]
    shapes = [[A, A, A, Bk], [B.bias[0], A, Bk, A], [A, Bk, A, Bk, A], [B.defs[0], B.bias[0], B.defs[0]], [B.bias[3], B.bias[3], A],
              [Cc, Bk, Cc], [B.bias[0], A, Bk], [B.defs[0], B.bias[0]], [Bk, Cc, B.defs[0], B.defs[0], B.defs[0]]]
    ex = []
    for c in range(3):
        for k, blocks in enumerate(shapes):
            ex.append([(b, block_values(b, 31 * c + 5 * k + j, 0.5)) for j, b in enumerate(blocks)])
    hdr, vals = pack(B.lay, ex, dtype)
    s = Set("dups", "mixed", hdr, vals, ids_in_groups(len(ex), 5, sizes=(3, 4)), seed=4, wreg=np.ones(B.L))
    s.tie_sensitive = True
    return s


# ---- exact cases on a power-of-two grid -------------------------------------------------------------------------------------
def exact_set():
    """C = 2^-9, wpos = 2, wreg = 1, w0 = 0, negatives whose x' are single powers of two (v = -x' / C), explicit orders.  Every
    product, sum and quotient below is exact, so each case is the same case in any summation order:
      E, E2     one bias value 2^-4, different ids: E's first step is free (a = 1/2); E2 then has Ai == 0 and G == 0 (none_lower,
                sv stays 1: the clear is strict); E in the second pass has G == 0
      S, T      one id: S = (2^-5, 2^-5, 0, 0) saturates its group in one step (a = b / d = 1 == maxA); T = (2^-5, 0, 0, 0) then pairs
                with it: dA = 1 == 1 - Ai == A2, both bounds
      H1 H2 H3  one id, one bias value 2^-4 each on their own coordinates: 1/2 + 1/2 is Ci == 1; H3 pairs with H2 (dA = 1/4, free)
      P, Q, Z   P, Q one id, 2^-5 on their own coordinates: P saturates (2 capped at 1), Q takes 1/2 from it; Z (another id,
                (-2^-5, 2^-6) on the two coordinates) then tilts w, and in the second pass Q gives back: dA = -3/4 held at
                -Ai == A2 - 1 == -1/2, both bounds (Q lies before P in the cache: a pass starts with idI at the group's highest
                index with a > 0)"""
    flat = mixed_model().flatten()
    B = Blocks(flat)
    p = lambda e: 2.0 ** e
    x = {
        "E": [(B.bias[1], [p(-4)])], "E2": [(B.bias[1], [p(-4)])],
        "S": [(B.defs[0], [p(-5), p(-5), 0, 0])], "T": [(B.defs[0], [p(-5), 0, 0, 0])],
        "H1": [(B.bias[2], [p(-4)])], "H2": [(B.bias[3], [p(-4)])], "H3": [(B.bias[6], [p(-4)])],
        "Q": [(B.bias[5], [p(-5)])], "P": [(B.bias[4], [p(-5)])], "Z": [(B.bias[4], [-p(-5)]), (B.bias[5], [p(-6)])],
    }
    names = list(x)
    group = {"E": 1, "E2": 2, "S": 3, "T": 3, "H1": 4, "H2": 4, "H3": 4, "P": 5, "Q": 5, "Z": 6}
    ex = [[(b, -np.asarray(v, np.float64) / C_GRID) for b, v in x[n]] for n in names]
    hdr, vals = pack(B.lay, ex)
    ids = np.zeros((len(ex), 5), np.int32)
    ids[:, 0] = -1
    ids[:, 1] = [group[n] for n in names]
    s = Set("exact", "mixed", hdr, vals, ids, passes=4, C=C_GRID, wpos=2.0, wreg=np.ones(B.L), w0=np.zeros(B.L))
    s.names = names
    at = {n: k for k, n in enumerate(names)}
    s.orders = [[at[n] for n in ("E", "E2", "S", "T", "H1", "H2", "H3", "P", "Q", "Z")],
                [at[n] for n in ("E", "E2", "Q", "P", "S", "T", "H1", "H2", "H3", "Z")]]
    s.orders += [s.orders[0][::-1], s.orders[1]]       # two more passes from where the cases left the duals
    return s


# ---- write edges ------------------------------------------------------------------------------------------------------------
def edge_set():
    """for T = double handles: values whose (C v) / wreg is an exact float32 halfway case with the kept bit even and odd, at
    normal and subnormal magnitudes, both signs; wreg with negative and non-unit entries; w0 non-zero on filter coordinates"""
    flat = mixed_model().flatten()
    B = Blocks(flat)
    A, D0 = B.filt[288][0], B.defs[0]
    u = 2.0 ** -24
    halves = np.array([1 + u, 1 + 3 * u, 1 + 5 * u, 1 + 7 * u, 2 - u, 2 - 3 * u, 1 + u + u * 2.0 ** -28, 1 + u - u * 2.0 ** -28])
    sub = np.array([2.0 ** -140, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -151, 2.0 ** -127 + 2.0 ** -150,
                    2.0 ** -126 - 2.0 ** -150, 5 * 2.0 ** -150])
    fa = np.zeros(288)
    fa[:8], fa[8:16] = halves, -halves
    fa[16:24], fa[24:32] = sub, -sub
    fa[32:64] = 0.25 * synth.normalish(5, 32, stream=1)
    fa[64:72] = halves * 2.0 ** -60
    wreg = np.ones(B.L)
    wreg[A[0] + 40:A[0] + 48] = [-1.0, -0.5, 3.0, 0.1, -7.0, 1e-3, 2.0 ** 20, -2.0 ** -20]
    wreg[A[0] + 64:A[0] + 72] = 2.0 ** -60      # (C v) / wreg is the halfway case, C v is not
    wreg[D0[0] + 1] = -3.0
    w0 = np.zeros(B.L)
    w0[A[0]:A[0] + 64] = 0.125 * synth.normalish(6, 64, stream=2)
    w0[D0[0]] = w0[D0[0] + 2] = 0.01
    ex = []
    for sign, Cl in ((1.0, C_GRID * 2.0), (-1.0, C_GRID)):          # a positive and a negative: x' = (Cl * (+-v)) / wreg
        for k in range(3):
            ex.append([(B.bias[k], [1.0]), (D0, [-4.0, -2.0, -1.0, 1.0]), (A, sign * fa / Cl)])
    ex.append([(A, fa / C_GRID), (A, np.zeros(288))])
    hdr, vals = pack(B.lay, ex)
    ids = np.zeros((len(ex), 5), np.int32)
    ids[:, 0] = [1, 1, 1, -1, -1, -1, -1]
    ids[:, 1] = [0, 1, 2, 7, 7, 7, 8]
    s = Set("edges", "mixed", hdr, vals, ids, passes=4, seed=6, C=C_GRID, wpos=2.0, wreg=wreg, w0=w0)
    return s


# ---- headers --------------------------------------------------------------------------------------------------------------
SLOTS_N = 2100
SLOTS_INVALID = (63, 64, 1023, 1024)
SLOTS_RUN = (1040, 2064)            # a whole run of 1024 marked-invalid headers


def slots_call(stride):
    """a call of SLOTS_N examples of nv <= 5 on the mixed model, with the marked-invalid headers above, records of `stride`
    words for the device route (ids = Q.ids_of_records(records, label, id_base)) and headers that are not examples of the layout
    (`foreign`, to be put in by the device test: pbd_qp_add refuses them).  Returns hdr, values (float64), records, foreign: a
    dict example -> header row"""
    flat = mixed_model().flatten()
    B = Blocks(flat)
    lay = B.lay
    ex = []
    for i in range(SLOTS_N):
        k = i % 3
        blocks = [[B.bias[i % len(B.bias)]], [B.defs[i % len(B.defs)]], [B.bias[(i // 3) % len(B.bias)], B.defs[(i // 5) % len(B.defs)]]][k]
        ex.append([(b, block_values(b, i, 1.0) * (1 + i % 4)) for b in blocks])
    hdr, vals = pack(lay, ex)
    for i in list(SLOTS_INVALID) + list(range(*SLOTS_RUN)):
        hdr[i] = invalid_header(lay, i)
    rec = np.zeros((SLOTS_N, stride), np.int32)
    rec[:, 0] = np.arange(SLOTS_N) // 4        # frame: id groups of four
    rec[:, 2] = np.arange(SLOTS_N) % 3
    rec[:, 3] = (np.arange(SLOTS_N) // 4) % 11
    rec[:, 4] = 7
    foreign = {}
    for i, (nb, nv, words) in {5: (1, 1, [B.bias[0][0], 2]), 70: (1, 4, [B.defs[0][0] + 1, 4]), 700: (2, 6, [0, 1, B.defs[0][0], 4]),
                               1030: (lay.MB + 1, 1, [0, 1]), 1033: (-2, 0, []), 2070: (1, 1, [B.L, 1]), 2071: (1, lay.V + 1, [0, 1]),
                               2072: (1, 1, [-1, 1])}.items():
        h = np.zeros(lay.in_hw, np.int32)
        h[:4] = (i, 0, nb, nv)
        h[4:4 + len(words)] = words
        foreign[i] = h
    return hdr, vals, rec, foreign


def all_sets():
    """every pass set: name -> Set.  shapes (default wreg: root biases at 0.01), shapes_w1 (wreg = 1, values at 1/4: groups
    saturate), dups, one_id, exact, edges"""
    B = Blocks(mixed_model().flatten())
    sets = [shape_set("shapes", scale=1.0, seed=1),
            shape_set("shapes_w1", scale=0.25, seed=2, wreg=np.ones(B.L)),
            dup_set(), one_id_set(), exact_set(), edge_set()]
    return {s.name: s for s in sets}


def run_ref(s, q=None, passes=None, each=None):
    """the set's passes on a QPRef (or a subclass instance): add, then one() per pass; the details of every step.  each(t, q) is
    called after every pass"""
    q = s.ref() if q is None else q
    assert q.add(s.hdr, s.values, s.ids) == int(np.sum(s.hdr[:, 2] >= 0))
    detail = []
    for t in range(s.passes if passes is None else passes):
        q.one(order=s.order(t, q.sv))
        detail += q.detail
        if each is not None:
            each(t, q)
    return q, detail
