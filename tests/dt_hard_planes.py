"""Score planes and models that drive the distance transform (include/DistanceTransform.hpp:152-182, computeRow) into the paths
ordinary data barely reaches -- deep envelopes, long pop runs, exact ties -- and a replay of computeRow that measures what a
plane does to it.  Shared by tests/test_gpu_dt_planes.py (every kernel variant against the oracle) and tests/test_oracle_cpu.py
(the oracle against brute force on the same planes); the planes with infinite and NaN scores by tests/test_gpu_dt_nonfinite.py and
tests/test_dt_nonfinite_cpu.py."""
import numpy as np

from partsbaseddetector_amd import model as M

KINDS = ("normal", "constant", "smooth", "spikes", "quantised", "wide")


def plane(kind, rng, h, w, big=1e20):
    """One (h, w) float64 score plane of the given kind; every value is exactly representable in float32 (and, for |big| <=
    65504, the kinds other than "normal", "smooth" and "wide" in fp16 too)."""
    if kind == "normal":
        p = rng.standard_normal((h, w))
    elif kind == "constant":                      # a concave quadratic keeps every element on the envelope: depth = row length
        p = np.full((h, w), float(rng.choice([0.75, -1.5, 0.0])))
    elif kind == "smooth":                        # deep envelopes with occasional pops
        y, x = np.mgrid[0:h, 0:w]
        p = 1e-3 * rng.standard_normal((h, w)) + 0.002 * x - 0.0015 * y
    elif kind == "spikes":                        # plateaus with isolated spikes of both signs every 20-40 cells
        p = np.full(h * w, 0.5)
        i = int(rng.integers(0, 20))
        while i < h * w:
            p[i] = float(rng.choice([-1.0, 1.0]) * rng.integers(3, 9))
            i += int(rng.integers(20, 41))
        p = p.reshape(h, w)
    elif kind == "quantised":                     # small integers or multiples of 1/4: exact ties with power-of-two quadratics
        step = 1.0 if rng.random() < 0.5 else 0.25
        p = rng.integers(-3, 4, (h, w)) * step
    elif kind == "wide":                          # +-1e-20 next to +-1e20: the intersection's rounding to float decides ties
        mag = rng.choice([1e-20, 1.0, big], size=(h, w), p=[0.45, 0.45, 0.1])
        p = mag * rng.choice([-1.0, 1.0], size=(h, w))
    else:
        raise ValueError(kind)
    return p.astype(np.float32).astype(np.float64)


def level_scores(nfilters, dims, seed, dtype=np.float32, big=1e20):
    """dims: [(h, w, kind or None)]; None gives filter f of level l the kind KINDS[(f + l) % 6]."""
    rng = np.random.default_rng(seed)
    out = []
    for l, (h, w, kind) in enumerate(dims):
        out.append(np.stack([plane(kind or KINDS[(f + l) % len(KINDS)], rng, h, w, big) for f in range(nfilters)]).astype(dtype))
    return out


# ---- planes with infinite and NaN scores (include/pbd.h, pbd_dp_min: "Non-finite scores") -----------------------------------
# Class F: no NaN intersection forms anywhere in the dynamic program, so every output is the reference's.  Class N: one does.
# Which class a plane falls into is measured by the callers (the oracle's count of NaN intersections), not assumed here.
NONFINITE_F = ("neg_holes", "pos_spikes", "f16_sat")
NONFINITE_N = ("neg_region", "pos_pair", "nan_cells")
F16_SAT = 7e4       # finite in float, beyond fp16's largest finite value (65504; from 65520 on it rounds to infinity)


def _holes(rng, h, w, density=0.15):
    """Isolated cells of an (h, w) plane, never two neighbouring along a row, so every row of two or more cells keeps another
    cell (a single-cell row gets none); with the first cell of the first row and the last cell of the last row among them."""
    m = rng.random((h, w)) < density
    if w < 2:
        return np.zeros((h, w), bool)
    m[0, 0] = True
    for x in range(1, w):
        m[:, x] &= ~m[:, x - 1]
    if w > 2 or h > 1:
        m[h - 1, w - 2], m[h - 1, w - 1] = False, True
    return m


def nonfinite_plane(kind, rng, h, w, spike=True, base="quantised"):
    """One (h, w) float64 plane of `base` kind ("quantised": exact in fp16 too) with the non-finite cells of `kind`.
    neg_holes: isolated -Inf cells (_holes).  pos_spikes: ONE +Inf cell when `spike` -- its row leaves the rows pass all +Inf, and
    a second such row anywhere in the plane would meet it in every column as Inf - Inf.  f16_sat: the same cells as those two
    kinds, at -+7e4: finite here, infinite once rounded to fp16.  neg_region: a rectangle of -Inf of 3 x 3 cells or more and one
    whole row and one whole column of -Inf (all clipped to the plane): a mask.  pos_pair: two +Inf neighbouring in a row and two
    in a column.  nan_cells: isolated NaN cells, the first cell of a row and the last cell of a row among them."""
    p = plane(base, rng, h, w)
    if kind in ("neg_holes", "f16_sat"):
        p[_holes(rng, h, w)] = -np.inf if kind == "neg_holes" else -F16_SAT
    if kind in ("pos_spikes", "f16_sat") and spike:
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        if kind == "pos_spikes" or p[y, x] != -F16_SAT:
            p[y, x] = np.inf if kind == "pos_spikes" else F16_SAT
    if kind == "neg_region":
        y0, x0 = int(rng.integers(0, max(h - 3, 1))), int(rng.integers(0, max(w - 3, 1)))
        p[y0:y0 + 3 + int(rng.integers(0, 3)), x0:x0 + 3 + int(rng.integers(0, 5))] = -np.inf
        p[int(rng.integers(0, h)), :] = -np.inf
        p[:, int(rng.integers(0, w))] = -np.inf
    if kind == "pos_pair":
        y, x = int(rng.integers(0, h)), int(rng.integers(0, max(w - 1, 1)))
        p[y, x:x + 2] = np.inf
        y, x = int(rng.integers(0, max(h - 1, 1))), int(rng.integers(0, w))
        p[y:y + 2, x] = np.inf
    if kind == "nan_cells":
        p[_holes(rng, h, w, 0.04)] = np.nan         # sparse: no pop run crosses a NaN entry, and some should be long
    if kind not in NONFINITE_F + NONFINITE_N:
        raise ValueError(kind)
    return p


def root_child_filters(flat):
    """Filter ids of the mixtures of every part whose parent is its component's root."""
    out = set()
    for c in range(flat.ncomponents):
        p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
        for g in range(p0 + 1, p1):
            if int(flat.parentid[g]) == 0:
                out |= {int(flat.filterid[gm]) for gm in range(int(flat.mix_offset[g]), int(flat.mix_offset[g + 1]))}
    return out


def nonfinite_scores(flat, kind, dims, seed, dtype=np.float32):
    """dims: [(h, w, base kind)] -> per level (nfilters, h, w) planes of the given non-finite kind.  The +Inf cell of pos_spikes and f16_sat
    goes to every other filter of the parts that are children of a root only: such a part's transform is +Inf everywhere, its
    parent's accumulated plane with it, and one generation higher a transform would run on rows of +Inf alone."""
    rng = np.random.default_rng(seed)
    spiked = root_child_filters(flat)
    return [np.stack([nonfinite_plane(kind, rng, h, w, spike=f in spiked and (f + l) % 2 == 0, base=base)
                      for f in range(flat.nfilters)]).astype(dtype) for l, (h, w, base) in enumerate(dims)]


# ---- models: small trees whose deformations are set after the model is built ----------------------------------------------
DEFORMATIONS = {
    "default": None,                                   # [0.01 0 0.01 0]: b = -0.0 in both passes (BZ)
    "linear": "linear",                                # synthetic linear terms: no BZ
    "xlinear": lambda mm: [0.01 + 0.002 * mm, 0.004 - 0.003 * mm, 0.012, 0.0],      # BZ in the columns pass only
    "pow2": lambda mm: [(0.25, 0.015625, 0.0625)[mm % 3], 0.0, (0.015625, 0.25, 0.0625)[mm % 3], 0.0],
    "pow2_linear": lambda mm: [(0.25, 0.015625, 0.0625)[mm % 3], (0.5, -0.25, 0.0)[mm % 3], 0.0625, (0.0, 0.125, -0.5)[mm % 3]],
}


def with_deformation(model, name):
    """Every deformation of mixture mm of every part becomes DEFORMATIONS[name](mm)."""
    fn = DEFORMATIONS[name]
    if callable(fn):
        for c in range(model.ncomponents()):
            for p in range(1, model.nparts(c)):
                for mm, d in enumerate(model.defid[c][p]):
                    model.defw[d] = [float(v) for v in fn(mm)]
        model.validate()
    return model


def dt_model(tree, deformation, thresh=0.0):
    linear = DEFORMATIONS[deformation] == "linear"
    if tree == "tiny":
        m = M.synthetic_tiny_model(thresh=thresh, linear_def=linear)
    else:   # five parts in three generations, three mixtures
        m = M.synthetic_model(seed=41, pa=[0, 1, 1, 2, 2], nmix=3, sbin=4, interval=4, thresh=thresh, linear_def=linear,
                              name="dt_tree")
    return with_deformation(m, deformation)


def leaf_jobs(flat):
    """(filter id, a_x, b_x, a_y, b_y, os_x, os_y) of every leaf part's mixtures: the transforms whose input is a raw plane."""
    jobs = []
    for c in range(flat.ncomponents):
        p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
        parents = {p0 + int(flat.parentid[g]) for g in range(p0 + 1, p1)}
        for g in range(p0 + 1, p1):
            if g in parents:
                continue
            for gm in range(int(flat.mix_offset[g]), int(flat.mix_offset[g + 1])):
                d = int(flat.defid[gm])
                w = flat.defw[d]
                jobs.append((int(flat.filterid[gm]), float(-w[0]), float(-w[1]), float(-w[2]), float(-w[3]),
                             int(flat.anchors[d][0]), int(flat.anchors[d][1])))
    return jobs


# ---- replay of computeRow on every row of a plane at once, with what it did -------------------------------------------------
def replay_rows(src, a, b, os0, R=np.float32, readout="reference"):
    """computeRow (DistanceTransform.hpp:152-182) on each row of src (M, N), in the oracle's arithmetic (double intersection
    rounded once to R).  readout: "reference" is computeRow's own loop (k = 0; while (z[k+1] < os) k++); "max" takes entry
    max{k : z[k] < os + q} of the finished envelope, a comparison with NaN being false (include/pbd.h, pbd_dp_min, rule 3) --
    found by looking at every entry, not by a walk.  Returns out (M, N) R, ptr (M, N) and per-row statistics: the deepest
    envelope (entries), the most entries popped for one element, whether an exact tie s == z[k] decided a pop-loop test (k > 0),
    whether z[k+1] == os decided a read-out test, nan_isect, the number of intersections pushed as NaN, top, the index of the
    finished envelope's top entry, and nan_floor, the index of its lowest entry with a NaN z (N + 2 where it has none)."""
    assert readout in ("reference", "max"), readout
    src = np.ascontiguousarray(src, R)
    Mr, N = src.shape
    rows = np.arange(Mr)
    v = np.zeros((Mr, N + 1), np.int64)
    z = np.full((Mr, N + 2), np.inf, R)
    z[:, 0] = -np.inf
    k = np.zeros(Mr, np.int64)
    depth = np.ones(Mr, np.int64)
    maxpop = np.zeros(Mr, np.int64)
    scan_tie = np.zeros(Mr, bool)
    read_tie = np.zeros(Mr, bool)
    nan_isect = np.zeros(Mr, np.int64)
    s64 = src.astype(np.float64)

    def isect(v0, q, sel):
        y0, y1 = s64[sel, v0], s64[sel, q]
        with np.errstate(all="ignore"):
            return (((y1 - y0) - b * (q - v0).astype(np.float64) + a * (q * q - v0 * v0).astype(np.float64))
                    / (2 * a * (q - v0).astype(np.float64))).astype(R)

    for q in range(1, N):
        s = isect(v[rows, k], q, rows)
        pops = np.zeros(Mr, np.int64)
        live = np.ones(Mr, bool)
        while True:
            zk = z[rows, k]
            with np.errstate(invalid="ignore"):
                scan_tie |= live & (k > 0) & (s == zk)
                m = live & (s <= zk) & (k > 0)
            if not m.any():
                break
            k[m] -= 1
            pops[m] += 1
            s[m] = isect(v[m, k[m]], q, m)
            live = m
        k += 1
        v[rows, k] = q
        z[rows, k] = s
        z[rows, k + 1] = np.inf
        nan_isect += np.isnan(s)
        depth = np.maximum(depth, k + 1)
        maxpop = np.maximum(maxpop, pops)
    out = np.empty((Mr, N), R)
    ptr = np.empty((Mr, N), np.int64)
    ktop = k
    k = np.zeros(Mr, np.int64)
    entry = np.arange(N + 2)
    isnan = np.isnan(z) & (entry[None, :] <= ktop[:, None])
    nan_floor = np.where(isnan.any(axis=1), isnan.argmax(axis=1), N + 2)
    for q in range(N):
        osf = R(os0 + q)
        if readout == "max":
            with np.errstate(invalid="ignore"):
                below = (z < osf) & (entry[None, :] <= ktop[:, None])     # entries above the top are stale
            k = N + 1 - np.argmax(below[:, ::-1], axis=1)                 # the last one; entry 0 (z = -inf) always qualifies
        while readout == "reference":
            zn = z[rows, k + 1]
            with np.errstate(invalid="ignore"):
                read_tie |= zn == osf
                m = zn < osf
            if not m.any():
                break
            k[m] += 1
        vk = v[rows, k]
        x = np.float64(os0 + q) - vk
        with np.errstate(invalid="ignore"):
            out[:, q] = ((a * (x * x) + b * x) + s64[rows, vk]).astype(R)
        ptr[:, q] = vk
    return out, ptr, {"depth": depth, "maxpop": maxpop, "scan_tie": scan_tie, "read_tie": read_tie, "nan_isect": nan_isect,
                      "top": ktop, "nan_floor": nan_floor}


def replay_dt(score, ax, bx, ay, by, osx, osy, R=np.float32, readout="reference"):
    """Both passes of one transform: the output (M, N) and the statistics of the rows pass and of the columns pass."""
    tmp, _, st_r = replay_rows(score, ax, bx, osx, R, readout)
    out, _, st_c = replay_rows(tmp.T, ay, by, osy, R, readout)
    return out.T, st_r, st_c
