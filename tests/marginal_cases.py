"""The cases of the max-marginal tests (test_marginals_cpu.py, test_gpu_marginals.py): small tree models, level sets and two sets
of values each.  The inputs are response planes handed to pbd_dp_min / marginals.max_marginals, so a case needs no image and its
levels can have any shape.

Hard cases (test_marginals_hard_cpu.py, test_gpu_marginals_hard.py).  "wide8" and "wide16" have parts of up to 8 and 16 types:
the two widest instantiations of k_mm_messages, reductions over more than 4 parent types, parent types of index 8 and above, and
for "wide16" mirrored transforms cut into one slice per parent type (part 1: 16 x 9 transforms, a slice holds 20) and into slices
of four parent types (part 2: 5 x 16).  The non-finite response sets give "tree" (dense values), "slices" and "wide16" (dyadic
values) the planes of tests/dt_hard_planes.py with +-Inf and NaN cells (every kind of NONFINITE_F and NONFINITE_N but f16_sat:
marginals are refused on fp16-resident responses) on the two level sets of tests/test_gpu_dt_nonfinite.py, base kinds unchanged:
test_marginals_hard_cpu.py shows that mirrored context planes built from them do spill the deepest ring ("i16") and do pop a
whole cooperative window ("u8").  Their yardstick is the rule with the "max" read-out.

Dyadic values: responses on the integer grid, deformation weights in quarters (linear terms of both signs and exactly 0), integer
biases, many of them equal so that ties occur; every sum the rule makes is then exact in float32 and float64.  Dense values:
random floats."""
from __future__ import annotations

import functools

import numpy as np

import dt_hard_planes as H
from test_gpu_dt_nonfinite import LEVELS as NF_LEVELS
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import marginals as MG
from partsbaseddetector_amd.model import Model

# one call holds a whole level set, so that flat lines cross level boundaries; 70 lines cross the 64-lane wave boundary
LEVELS_A = [(1, 1), (1, 9), (9, 1), (7, 9), (3, 70), (70, 3)]
LEVELS_B = LEVELS_A + [(2, 300)]          # a side above 256 forces int16 position planes
LEVEL_SETS = {"A": LEVELS_A, "B": LEVELS_B}

# name -> per component (1-based parent table as synth's, types per part, filter size per part, anchors per non-root part or None)
MODELS = {
    # K == 1 on both reductions: part 2 has one type (the message copies), its parent... and part 1's parent has two
    "chain": [dict(pa=[0, 1, 2], K=[2, 3, 1], ks=[5, 5, 5])],
    "chain1": [dict(pa=[0, 1, 2], K=[1, 2, 3], ks=[5, 5, 5])],     # a one-type parent: the K_q == 1 copy of the downward reduction
    "star": [dict(pa=[0, 1, 1, 1], K=[2, 2, 2, 2], ks=[5, 5, 5, 5])],
    # depth 3, up to 4 types, anchors of both signs and one beyond the 9-cell side, filters of three sizes
    "tree": [dict(pa=[0, 1, 1, 2, 2, 4], K=[3, 4, 2, 1, 4, 2], ks=[5, 3, 7, 5, 3, 5],
                  anchors={1: (-3, 2), 2: (11, -1), 3: (2, -2), 4: (-1, 3), 5: (0, -12)})],
    "two": [dict(pa=[0, 1], K=[2, 2], ks=[5, 5]), dict(pa=[0, 1, 1, 3], K=[1, 3, 2, 2], ks=[3, 5, 5, 3])],
    # part 1 alone at its depth: the scratch holds 3 transforms, its mirrored ones are 12, so every parent type is a slice of its own
    "slices": [dict(pa=[0, 1, 2], K=[4, 3, 2], ks=[5, 5, 5])],
    # up to 8 types: k_mm_messages<R, 8>, reductions over 8 parent types
    "wide8": [dict(pa=[0, 1, 1], K=[8, 5, 6], ks=[5, 5, 5])],
    # 16 types under a parent of 9, 5 under a parent of 16: k_mm_messages<R, 16>, Jk up to 15.  The scratch holds 20 transforms:
    # every parent type of part 1 is a slice of its own, parts 3 and 4 fill the slices' ends, part 2 resumes every 4 parent types.
    # Parts 3 and 4 give part 1 two siblings, so that the order of their messages matters.
    "wide16": [dict(pa=[0, 1, 2, 1, 1], K=[9, 16, 5, 2, 2], ks=[5, 5, 5, 5, 5])],
}
CASES = [(m, ls) for m in ("chain", "star", "tree", "two", "slices") for ls in ("A", "B")] + [("chain1", "A")]
VALUES = ("dyadic", "dense")
WIDE_CASES = [("wide8", "A"), ("wide16", "B")]          # not in CASES: the existing tests' parametrisation stays as it is

# the non-finite cases: (model, its value set); every kind on both level sets
NF_MODELS = [("tree", "dense"), ("slices", "dyadic"), ("wide16", "dyadic")]
NF_KINDS = tuple(k for k in H.NONFINITE_F + H.NONFINITE_N if k != "f16_sat")
NF_SETS = tuple(NF_LEVELS)


@functools.lru_cache(maxsize=None)
def model(name: str, values: str) -> Model:
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + (values == "dense"))
    m = Model(name=f"marginal_{name}_{values}", interval=2, thresh=0.0)
    dy = values == "dyadic"
    for comp in MODELS[name]:
        pa, K, ks = comp["pa"], comp["K"], comp["ks"]
        fid_c, bid_c, did_c = [], [], []
        for p in range(len(pa)):
            fid = []
            for _ in range(K[p]):
                fid.append(len(m.filtersw))
                m.filtersw.append(rng.standard_normal((ks[p], ks[p] * 32)) * 0.05)
            fid_c.append(fid)
            if pa[p] == 0:
                bid_c.append([len(m.biasw)])
                m.biasw.append(float(rng.integers(-2, 3)) if dy else float(rng.standard_normal() * 0.5))
                did_c.append([])
                continue
            L = K[pa[p] - 1]
            base = len(m.biasw)
            m.biasw.extend([float(v) for v in (rng.integers(-1, 2, K[p] * L) if dy else rng.standard_normal(K[p] * L) * 0.5)])
            bid_c.append([base + mm * L for mm in range(K[p])])
            dids = []
            for mm in range(K[p]):
                dids.append(len(m.defw))
                if dy:
                    lin = [-0.5, -0.25, 0.0, 0.25, 0.5]
                    m.defw.append([float(rng.integers(1, 5)) / 4, lin[int(rng.integers(0, 5))], float(rng.integers(1, 5)) / 4,
                                   lin[int(rng.integers(0, 5))]])
                else:
                    m.defw.append([float(rng.uniform(0.01, 0.2)), float(rng.normal() * 0.05), float(rng.uniform(0.01, 0.2)),
                                   float(rng.normal() * 0.05)])
                a = comp.get("anchors", {}).get(p)
                if a is None or mm > 0:
                    a = (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
                m.anchors.append(a)
            did_c.append(dids)
        m.filterid.append(fid_c)
        m.biasid.append(bid_c)
        m.defid.append(did_c)
        m.parentid.append([q - 1 for q in pa])
    m.validate()
    return m


@functools.lru_cache(maxsize=None)
def responses(name: str, levels: str, values: str, dtype: str):
    """per level (nfilters, H, W) of dtype; the same numbers for float32 and float64"""
    nf = model(name, values).nfilters()
    rng = np.random.default_rng(sum(map(ord, name + levels)) + 13 * (values == "dense"))
    out = []
    for H, W in LEVEL_SETS[levels]:
        if values == "dyadic":
            r = rng.integers(-4, 5, (nf, H, W)).astype(np.float32)
        else:
            r = rng.standard_normal((nf, H, W)).astype(np.float32)
        out.append(np.ascontiguousarray(r.astype(dtype)))
    return out


def scales(levels: str) -> np.ndarray:
    return np.array([1.0 + 0.37 * l for l in range(len(LEVEL_SETS[levels]))], np.float32)


@functools.lru_cache(maxsize=None)
def yardstick(name: str, levels: str, values: str, dtype: str):
    """per level, per component: dict(mm, down, Jx, Jy, Jk, IxRaw, IyRaw, Ik, rootv, rooti); computed once, never written to"""
    flat = model(name, values).flatten()
    out = []
    for resp in responses(name, levels, values, dtype):
        per_c = []
        for c in range(flat.ncomponents):
            mm, down, Jx, Jy, Jk = MG.max_marginals(flat, c, resp)
            IxRaw, IyRaw, Ik, rootv, rooti = E.raw_maps(flat, c, resp)
            d = dict(mm=mm, down=down, Jx=Jx, Jy=Jy, Jk=Jk, IxRaw=IxRaw, IyRaw=IyRaw, Ik=Ik, rootv=rootv, rooti=rooti)
            for v in d.values():
                v.setflags(write=False)
            per_c.append(d)
        out.append(per_c)
    return out


def merged(name: str, levels: str, values: str, dtype: str, key: str):
    """per level the (NJ, H, W) block of all components together, as pbd_get_marginals returns it"""
    flat = model(name, values).flatten()
    out = []
    for per_c in yardstick(name, levels, values, dtype):
        a = np.array(per_c[0][key], copy=True)
        for c in range(1, flat.ncomponents):
            g0, g1 = int(flat.mix_offset[flat.part_offset[c]]), int(flat.mix_offset[flat.part_offset[c + 1]])
            a[g0:g1] = per_c[c][key][g0:g1]
        out.append(a)
    return out


def part_planes(flat, c: int, p: int):
    g = int(flat.part_offset[c]) + p
    return range(int(flat.mix_offset[g]), int(flat.mix_offset[g + 1]))


def seeds_of(name: str, levels: str, values: str, dtype: str):
    """the decode's seeds: every part's best cell on the 7 x 9 level (its own type, then type -1), the four corners of the 3 x 70
    level with type -1, and a few bad seeds"""
    flat = model(name, values).flatten()
    ys = yardstick(name, levels, values, dtype)
    seeds = []
    for c in range(flat.ncomponents):
        n = int(flat.part_offset[c + 1]) - int(flat.part_offset[c])
        for p in range(n):
            for l in (3, 5):
                pl = list(part_planes(flat, c, p))
                blk = ys[l][c]["mm"][pl[0]:pl[-1] + 1]
                t, y, x = np.unravel_index(int(np.argmax(blk)), blk.shape)
                seeds += [(l, c, p, int(t), int(x), int(y)), (l, c, p, -1, int(x), int(y))]
        H, W = LEVEL_SETS[levels][4]
        for (x, y) in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            seeds.append((4, c, n - 1, -1, x, y))
    H, W = LEVEL_SETS[levels][3]
    nl = len(LEVEL_SETS[levels])
    bad = [(3, 0, 0, 0, W, 0), (3, 0, 0, 0, 0, H), (3, 0, 0, 0, -1, 0), (nl, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (3, flat.ncomponents, 0, 0, 0, 0),
           (3, 0, 99, 0, 0, 0), (3, 0, 0, 16, 0, 0), (3, 0, 0, -2, 0, 0)]
    return np.asarray(seeds[:3] + bad[:4] + seeds[3:] + bad[4:], np.int32)


def decode_all(name: str, levels: str, values: str, dtype: str, seeds, frame_offset: int = 0, fill: int = 0):
    """(status, records, place) marginals.decode gives for the seeds, as Handle.marginal_poses returns them"""
    return decode_seeds(model(name, values).flatten(), yardstick(name, levels, values, dtype), LEVEL_SETS[levels], scales(levels),
                        dtype, seeds, frame_offset, fill)


def decode_seeds(flat, ys, shapes, sc, dtype: str, seeds, frame_offset: int = 0, fill: int = 0):
    """decode_all on a yardstick ys (per level, per component, the dict of yardstick()) of levels of the given shapes and scales"""
    n, mp = len(seeds), int(flat.max_parts)
    status = np.full(n, fill, np.int32)
    rec = np.full((n, 8 + 4 * mp), fill, np.int32)
    place = np.full((n, mp, 3), fill, np.int32)
    for i, s in enumerate(seeds):
        if not MG.seed_valid(flat, shapes, s):
            status[i] = -1
            continue
        l, c, p, t, x, y = (int(v) for v in s)
        d = ys[l][c]
        pl, r = MG.decode(flat, c, l, p, t, x, y, d["mm"], d["Jx"], d["Jy"], d["Jk"], d["IxRaw"], d["IyRaw"], d["Ik"], sc[l], 0,
                          frame_offset, np.dtype(dtype))
        k = len(pl)
        status[i] = k
        rec[i, :8 + 4 * k] = r[:8 + 4 * k]
        place[i, :k] = np.asarray(pl, np.int32)
    return status, rec, place


# ---- the non-finite cases ----------------------------------------------------------------------------------------------------
def nf_values(name: str) -> str:
    return dict(NF_MODELS)[name]


@functools.lru_cache(maxsize=None)
def nf_responses(name: str, kind: str, set_name: str, dtype: str):
    """per level (nfilters, H, W) of dtype: dt_hard_planes.nonfinite_scores on the level set, seeded as the DT suite seeds it"""
    flat = model(name, nf_values(name)).flatten()
    seed = 1000 * (H.NONFINITE_F + H.NONFINITE_N).index(kind) + {"u8": 11, "i16": 22}[set_name] + sum(map(ord, name))
    return H.nonfinite_scores(flat, kind, NF_LEVELS[set_name], seed, np.dtype(dtype).type)


def nf_shapes(set_name: str):
    return [(h, w) for h, w, _ in NF_LEVELS[set_name]]


def nf_scales(set_name: str) -> np.ndarray:
    return np.array([1.0 + 0.37 * l for l in range(len(NF_LEVELS[set_name]))], np.float32)


@functools.lru_cache(maxsize=None)
def nf_yardstick(name: str, kind: str, set_name: str, dtype: str, readout: str = "max"):
    """(per level, per component the dict of yardstick(); NaN intersections {"upward", "mirrored"} of all levels together) under
    the given read-out; computed once, never written to"""
    flat = model(name, nf_values(name)).flatten()
    out, nans = [], {}
    for resp in nf_responses(name, kind, set_name, dtype):
        per_c = []
        for c in range(flat.ncomponents):
            mm, down, Jx, Jy, Jk = MG.max_marginals(flat, c, resp, readout=readout, nan_isect=nans)
            IxRaw, IyRaw, Ik, rootv, rooti = E.raw_maps(flat, c, resp, readout=readout)
            d = dict(mm=mm, down=down, Jx=Jx, Jy=Jy, Jk=Jk, IxRaw=IxRaw, IyRaw=IyRaw, Ik=Ik, rootv=rootv, rooti=rooti)
            for v in d.values():
                v.setflags(write=False)
            per_c.append(d)
        out.append(per_c)
    return out, nans


def nf_cells(name: str, kind: str, set_name: str, dtype: str):
    """cells of the "max" yardstick a type -1 seed has to get right: ({"nan": seeds, "neginf": seeds, "finite": seeds}); "nan":
    for each part the first cell (level, then raster order) where the mm of every type is NaN, "neginf": where every one is -Inf,
    "finite": the cell of its largest finite mm of the first level that has one.  One-component models."""
    flat = model(name, nf_values(name)).flatten()
    ys = nf_yardstick(name, kind, set_name, dtype)[0]
    out = {"nan": [], "neginf": [], "finite": []}
    for p in range(int(flat.part_offset[1])):
        pl = list(part_planes(flat, 0, p))
        found = set()
        for l, per_c in enumerate(ys):
            blk = per_c[0]["mm"][pl[0]:pl[-1] + 1]
            tests = {"nan": np.isnan(blk).all(0), "neginf": np.isneginf(blk).all(0), "finite": np.isfinite(blk).any(0)}
            for key, t in tests.items():
                if key in found or not t.any():
                    continue
                found.add(key)
                if key == "finite":
                    b = np.where(np.isfinite(blk), blk, -np.inf)
                    _, y, x = np.unravel_index(int(np.argmax(b)), b.shape)
                else:
                    y, x = np.argwhere(t)[0]
                out[key].append((l, 0, p, -1, int(x), int(y)))
    return out


def nf_seeds(name: str, kind: str, set_name: str, dtype: str):
    """the decode's seeds of a non-finite case: the corners of the first level for the last part, nf_cells' (every part's best
    finite cell, all-NaN and all -Inf cells), all with type -1, the best finite cells again with type 0, and bad seeds in between"""
    flat = model(name, nf_values(name)).flatten()
    cells = nf_cells(name, kind, set_name, dtype)
    H0, W0 = nf_shapes(set_name)[0]
    last = int(flat.part_offset[1]) - 1
    seeds = [(0, 0, last, -1, x, y) for x, y in ((0, 0), (W0 - 1, 0), (0, H0 - 1), (W0 - 1, H0 - 1))]
    seeds += cells["finite"] + cells["nan"] + cells["neginf"] + [(l, c, p, 0, x, y) for l, c, p, _, x, y in cells["finite"]]
    nl = len(NF_LEVELS[set_name])
    bad = [(0, 0, 0, 0, W0, 0), (0, 0, 0, 0, 0, H0), (0, 0, 0, 0, -1, 0), (nl, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (0, flat.ncomponents, 0, 0, 0, 0),
           (0, 0, 99, 0, 0, 0), (0, 0, 0, 16, 0, 0), (0, 0, 0, -2, 0, 0)]
    return np.asarray(seeds[:3] + bad[:4] + seeds[3:] + bad[4:], np.int32)
