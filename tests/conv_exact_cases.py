"""The built inputs the exact convolution (PBD_CONV_EXACT: k_conv3<false, NW> and k_conv_generic<float|double, false, 5|0>,
csrc/pbd_kernels_conv.hip) is pinned on, a plain numpy statement of its arithmetic, and restatements of the host rules that
choose the kernel variant.  Shared by tests/test_conv_exact_cpu.py (the oracle against the plain statement, what the inputs
discriminate, which variants they reach -- no GPU) and tests/test_gpu_conv_exact.py (the kernels against the oracle, bit for bit).

LEVELS.  CONV3_LEVELS is cut for k_conv3's strips of four rows and 64-position tiles of up to three segments: heights with
H % 4 = 0..3, widths 1, 2, 63, 64, 65, 130, maps smaller than the filter, an empty level between non-empty ones and a run of
narrow one-strip levels that one tile takes as three segments of three levels.  GENERIC_LEVELS is cut for k_conv_generic's 32 x 8
tiles: sides 1, 7, 8, 9, 31, 32, 33, large paired with small, and a 1 x 2 map smaller than every filter but K = 1.  LARGE_LEVELS
is one long level whose cover has at least 1024 workgroups, where launch_conv_stage stops splitting units / filter groups over
blockIdx.y.  REDUCED_* are the few small levels the numpy statement is run on.

WEIGHTS.  hard_filters(): magnitudes 10^u, u uniform in [-4, 2), both signs, about 6 % exact +0 and 3 % -0 per filter, so that
another tap or channel order, a fused multiply-add or a missing per-channel sum changes the bits of most responses (measured in
tests/test_conv_exact_cpu.py).  FEATURES: uniform in [0, 0.4) like HOG, channel 31 = 0 unless a case says otherwise.

Everything is seeded; a case is computed once per process and frozen (setflags(write=False))."""
import functools
import os
import re

import numpy as np

from partsbaseddetector_amd import model as MD
from partsbaseddetector_amd import synth

FLEN = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")

CONV3_LEVELS = [(8, 63), (5, 64), (6, 65), (7, 130), (9, 1), (4, 2), (3, 2), (1, 1), (0, 5), (1, 5), (2, 7), (3, 9), (12, 21)]
GENERIC_LEVELS = [(1, 33), (7, 32), (8, 31), (9, 9), (31, 8), (32, 7), (33, 1), (1, 2)]
LARGE_LEVELS = [(9, 16401), (3, 2)]
REDUCED_CONV3 = [(5, 7), (3, 2), (1, 1), (0, 5), (6, 3)]
REDUCED_GENERIC = [(4, 5), (1, 2), (3, 1)]
C31_LEVELS = (0, 3)            # levels of a list whose channel 31 is made non-zero inside the map (the pdf path computes it)

# 5 x 5 float banks: filter counts (units: test_conv_exact_cpu.py asserts that 8, 6, 4 and 2 all occur and that a bank is odd)
CONV3_BANKS = [1, 8, 9, 17, 51]
# a 5 x 5 class inside a mixed bank: ids 1, 3, 5 of 7 filters -> non-identity fmap, an odd class
MIXED_SIZES = [3, 5]
MIXED_COUNT = 7
# generic banks: (K, filter count) at both edges of every cblock bucket; the counts cover 1, 8, 9, 17 for either type
GENERIC_BANKS = [(1, 17), (2, 9), (7, 8), (8, 17), (16, 1), (17, 9), (30, 8), (31, 1)]
GENERIC_BANKS_F64 = GENERIC_BANKS + [(5, 9)]
LARGE_BANK_CONV3 = 17
LARGE_BANK_GENERIC = (2, 17)


def _freeze(a):
    a.setflags(write=False)
    return a


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def hard_filter(rng, k, dtype=np.float32):
    """(k, k*32): magnitudes over six decades, both signs, exact zeros and negative zeros"""
    n = k * k * FLEN
    w = (10.0 ** rng.uniform(-4.0, 2.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    u = rng.random(n)
    w = np.where(u < 0.06, 0.0, w)
    w = np.where((u >= 0.06) & (u < 0.09), -0.0, w)
    return np.ascontiguousarray(w.astype(dtype).reshape(k, k * FLEN))


def features(rng, h, w, dtype=np.float32, c31=None):
    """(h, w*32) uniform in [0, 0.4); channel 31 = 0, or uniform in [0, c31)"""
    f = (rng.random((h, w * FLEN)) * 0.4).astype(dtype)
    if f.size:
        v = f.reshape(h, w, FLEN)
        v[:, :, FLEN - 1] = 0 if c31 is None else (rng.random((h, w)) * c31).astype(dtype)
    return np.ascontiguousarray(f)


@functools.lru_cache(maxsize=None)
def level_features(which, dtype_name):
    """the frozen feature maps of a level list ("conv3", "generic", "large", "reduced_conv3", "reduced_generic"); channel 31 is
    non-zero inside the map on the levels C31_LEVELS"""
    dims = {"conv3": CONV3_LEVELS, "generic": GENERIC_LEVELS, "large": LARGE_LEVELS, "reduced_conv3": REDUCED_CONV3,
            "reduced_generic": REDUCED_GENERIC}[which]
    rng = np.random.default_rng(9000 + sorted(["conv3", "generic", "large", "reduced_conv3", "reduced_generic"]).index(which))
    dt = np.dtype(dtype_name).type
    return tuple(_freeze(features(rng, h, w, dt, c31=0.3 if (l in C31_LEVELS and which != "large") else None))
                 for l, (h, w) in enumerate(dims))


@functools.lru_cache(maxsize=None)
def bank(sizes, dtype_name, seed=0):
    """the frozen filters of a bank: sizes = tuple of filter sides"""
    rng = np.random.default_rng(100 + 7 * len(sizes) + 1000 * sizes[0] + seed)
    return tuple(_freeze(hard_filter(rng, k, np.dtype(dtype_name).type)) for k in sizes)


def mixed_sizes():
    return tuple(MIXED_SIZES[i % len(MIXED_SIZES)] for i in range(MIXED_COUNT))


@functools.lru_cache(maxsize=None)
def zero_case(k, dtype_name):
    """(features, filters): an all-zero level (and a non-zero one) under three filters whose weights are all negative, and -0 on
    channel 31"""
    dt = np.dtype(dtype_name).type
    rng = np.random.default_rng(40 + k)
    filters = []
    for _ in range(3):
        w = -np.abs(hard_filter(rng, k, dt)) - dt(1e-3)
        w.reshape(k * k, FLEN)[:, FLEN - 1] = -0.0          # (the border of channel 31 is 1: its taps would not give 0)
        filters.append(_freeze(w))
    filters = tuple(filters)
    feats = (_freeze(np.zeros((6, 9 * FLEN), dt)), _freeze(features(rng, 5, 4, dt)), _freeze(np.zeros((1, 1 * FLEN), dt)))
    return feats, filters


@functools.lru_cache(maxsize=None)
def subnormal_case(k, dtype_name):
    """(features, filters) whose products are subnormal in the response type: float weights near 1e-30 against features near
    1e-10 (products near 1e-40 < 1.18e-38), double 1e-200 against 1e-110 (1e-310 < 2.2e-308); sums of 32 k k of them stay
    subnormal, so a unit that flushes subnormal results or operands to zero gives 0 where the oracle (CPU, subnormals kept)
    does not"""
    dt = np.dtype(dtype_name).type
    rng = np.random.default_rng(50 + k)
    ws, fs = (1e-30, 1e-10) if dt == np.float32 else (1e-200, 1e-110)
    n = k * k * FLEN
    filters = []
    for _ in range(3):
        w = ((0.5 + rng.random(n)) * ws * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(dt).reshape(k * k, FLEN)
        w[:, FLEN - 1] = 0                                  # (the border of channel 31 is 1: its products would be normal)
        filters.append(_freeze(np.ascontiguousarray(w.reshape(k, k * FLEN))))
    filters = tuple(filters)
    feats = tuple(_freeze(((0.5 + rng.random((h, w * FLEN))) * fs).astype(dt)) for h, w in ((6, 9), (3, 2), (9, 70)))
    return feats, filters


# ---- the fused path's model -------------------------------------------------------------------------------------------------
# (69, 32) and (175, 169) are base shapes of tests/test_gpu_feature_variants.py (sbin 4): maps down to 9 x 3 and 4 x 4 cells.
# Their pyramids hold no 3-cell height and no map wide enough for a tile inside one strip, so three more: (32, 69) ends in a
# 3 x 9 map, (32, 32), the smallest frame accepted, in 3 x 3, and (64, 560) starts with 14 x 138 (wholly interior tiles).
FUSED_SHAPES = [(69, 32), (32, 69), (32, 32), (175, 169), (64, 560)]
FUSED_INTERVAL = 3
BATCH_SHAPE = (69, 32)
MIXED_SHAPES = [(69, 32), (175, 169), (40, 83)]
C31_MAGNITUDES = (1e3, 1.0, 1e-4)


@functools.lru_cache(maxsize=None)
def fused_model():
    """5 parts x 3 mixtures = 15 filters of 5 x 5 (an odd bank), the hard weights, and channel-31 weights of the 25 taps of mixed
    magnitude (1e3, 1, 1e-4 with a random mantissa, both signs), one exact zero and one -0 per filter: the ordered sum of the
    out-of-image taps differs in bits from the sorted, the reversed and the column-major sum"""
    m = MD.synthetic_model(seed=31, pa=[0, 1, 1, 2, 2], nmix=3, ksize=5, interval=FUSED_INTERVAL, thresh=1e9, name="conv-exact")
    rng = np.random.default_rng(77)
    for i in range(len(m.filtersw)):
        w = hard_filter(rng, 5, np.float32).astype(np.float64).reshape(25, FLEN)
        mag = np.array([C31_MAGNITUDES[int(v)] for v in rng.integers(0, 3, 25)])
        c31 = (mag * (1.0 + rng.random(25)) * np.where(rng.random(25) < 0.5, -1.0, 1.0)).astype(np.float32).astype(np.float64)
        z = rng.choice(25, 2, replace=False)
        c31[z[0]], c31[z[1]] = 0.0, -0.0
        w[:, FLEN - 1] = c31
        m.filtersw[i] = w.reshape(5, 5 * FLEN)
    m.validate()
    return m


def fused_frame(seed, shape):
    return synth.synthetic_frame(seed, shape[0], shape[1], 3)


# ---- the plain statement ----------------------------------------------------------------------------------------------------
def padded_planes(feat, k):
    """(32, H+k-1, W+k-1) channel planes with the constant border: 0, but 1 on the last channel; anchor k // 2"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    a = k // 2
    P = np.zeros((FLEN, H + k - 1, W + k - 1), feat.dtype)
    P[FLEN - 1] = 1
    P[:, a:a + H, a:a + W] = np.moveaxis(feat.reshape(H, W, FLEN), 2, 0)
    return P


def plain_conv(feat, filters, variant="exact"):
    """The reference's arithmetic in numpy, in the response type itself, for filters of one side k: (F, H, W).

    exact: per channel an accumulator starts at 0; for each tap in raster order with a non-zero weight acc = acc + w * plane
    (a rounded multiply, then a rounded add); a channel whose taps are all zero applies one 0 * plane tap at (0, 0); then
    resp = resp + acc in channel order.  The mutants: "fma" one rounding per tap (float32 only, through float64: the product
    of two floats is exact there), "colmajor" taps in column-major order, "revchan" channels 31..0, "direct" taps accumulated
    straight into the response without the per-channel sum."""
    dt = feat.dtype.type
    k = filters[0].shape[0]
    H, W = feat.shape[0], feat.shape[1] // FLEN
    F = len(filters)
    Wt = np.stack([np.asarray(f, dt).reshape(k, k, FLEN) for f in filters])          # (F, i, j, c)
    resp = np.zeros((F, H, W), dt)
    if H * W == 0:
        return resp
    P = padded_planes(feat, k)
    taps = [(i, j) for i in range(k) for j in range(k)]
    if variant == "colmajor":
        taps = [(i, j) for j in range(k) for i in range(k)]
    chans = range(FLEN - 1, -1, -1) if variant == "revchan" else range(FLEN)
    for c in chans:
        acc = resp if variant == "direct" else np.zeros((F, H, W), dt)
        nz = (Wt[:, :, :, c] != 0).reshape(F, -1).any(axis=1)
        for i, j in taps:
            w = Wt[:, i, j, c].reshape(F, 1, 1)
            src = P[c, i:i + H, j:j + W][None]
            if variant == "fma":
                assert dt == np.float32
                new = (w.astype(np.float64) * src.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            else:
                new = acc + w * src
            acc[...] = np.where(w != 0, new, acc)
        if not nz.all():
            zero_tap = acc + dt(0) * P[c, 0:H, 0:W][None]
            acc[...] = np.where(nz.reshape(F, 1, 1), acc, zero_tap)
        if variant != "direct":
            resp = resp + acc
    return resp


def plain_responses(feat, filters, variant="exact"):
    """plain_conv over a bank of mixed sizes, filter order kept"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    out = np.zeros((len(filters), H, W), feat.dtype)
    for k in sorted({f.shape[0] for f in filters}):
        ids = [i for i, f in enumerate(filters) if f.shape[0] == k]
        out[ids] = plain_conv(feat, [filters[i] for i in ids], variant)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def oracle_responses(oracle, feat, filters):
    """(F, H, W): oracle.conv of every filter on one level"""
    H, W = feat.shape[0], feat.shape[1] // FLEN
    if H * W == 0:
        return np.zeros((len(filters), H, W), feat.dtype)
    return np.stack([oracle.conv(feat, np.asarray(f, feat.dtype)) for f in filters])


# ---- channel-31 table ---------------------------------------------------------------------------------------------------
def c31_case(y, x, H, W):
    """the epilogue's case of output (y, x) of an H x W map: rows / columns of the 5 x 5 window outside, each clipped to 0..2"""
    a = 2
    clip = lambda v: min(max(v, 0), a)
    top, bot, left, right = clip(a - y), clip(y + a - (H - 1)), clip(a - x), clip(x + a - (W - 1))
    return ((top * 3 + bot) * 3 + left) * 3 + right


def c31_cases_of(dims):
    return {c31_case(y, x, H, W) for H, W in dims for y in range(H) for x in range(W)}


def c31_outside(cs, i, j):
    right, left, bot, top = cs % 3, cs // 3 % 3, cs // 9 % 3, cs // 27
    return i < top or i > 4 - bot or j < left or j > 4 - right


def c31_sum(w25, cs, order="raster"):
    """float32 sum of the non-zero channel-31 weights of the out-of-image taps of case cs, in the given order"""
    taps = [(i, j) for i in range(5) for j in range(5) if c31_outside(cs, i, j)]
    if order == "colmajor":
        taps = sorted(taps, key=lambda t: (t[1], t[0]))
    vals = [np.float32(w25[i * 5 + j]) for i, j in taps]
    if order == "reversed":
        vals = vals[::-1]
    if order == "sorted":
        vals = sorted(vals)
    s = np.float32(0)
    for v in vals:
        if v != 0:
            s = np.float32(s + v)
    return s


# ---- host rules restated ------------------------------------------------------------------------------------------------
def internal_constants():
    """kConvTW, kConvTH, kConvQ, kConvMaxK, kConvLdsBudget, kConv3NW read from csrc/pbd_internal.h"""
    text = open(os.path.join(CSRC, "pbd_internal.h")).read()
    out = {}
    m = re.search(r"constexpr int kConvTW = (\d+), kConvTH = (\d+), kConvQ = (\d+);", text)
    out["TW"], out["TH"], out["Q"] = (int(v) for v in m.groups())
    out["MaxK"] = int(re.search(r"constexpr int kConvMaxK = (\d+);", text).group(1))
    m = re.search(r"constexpr size_t kConvLdsBudget = (\d+) \* (\d+);", text)
    out["LdsBudget"] = int(m.group(1)) * int(m.group(2))
    out["NW"] = int(re.search(r"#define PBD_CONV3_NW (\d+)", text).group(1))
    return out


def cblock(K, itemsize, const=None):
    """launch_conv_stage: channels of the haloed tile staged at a time by k_conv_generic"""
    c = const or internal_constants()
    plane = (((c["TH"] + K - 1) * (c["TW"] + K - 1)) | 1) * itemsize
    cb = 32
    while cb > 1 and cb * plane > c["LdsBudget"]:
        cb //= 2
    return cb


def conv_units(nf, nw):
    """conv_units (csrc/pbd_capi.hip): the unit sizes k_conv3 cuts a bank of nf filters into"""
    P = (nf + 1) // 2
    best, pick = 1e30, (0, 0, 0)
    for a in range(P // 4, -1, -1):
        for c in range(3):
            rest = P - 4 * a - c
            if rest < 0 or rest % 3:
                continue
            b = rest // 3
            load = [0.0] * nw

            def give(n, cost):
                for _ in range(n):
                    load[load.index(min(load))] += cost
            give(a, 4 + 0.2)
            give(b, 3 + 0.2)
            if c:
                give(1, c + 0.2)
            span = max(load) + (0.01 if c else 0.0)
            if span < best - 1e-9:
                best, pick = span, (a, b, c)
    a, b, c = pick
    return [8] * a + [6] * b + ([2 * c] if c else [])


def generic_tiles(dims, const=None):
    """P.ntiles of a level list: the 32 x 8 tiles launch_conv_stage counts workgroups by"""
    c = const or internal_constants()
    return sum(-(-h // c["TH"]) * -(-w // c["TW"]) for h, w in dims if h * w)


def split(n, wgs):
    """units_per_block / groups_per_block of launch_conv_stage for n units / groups and wgs = ntiles * frames"""
    return max(n, 1) if wgs >= 1024 else max(1, n * wgs // 1024)


def seg_tiles(dims, nb):
    """pbd_debug_seg_tiles: (n, 16) int32 = nseg, len[3], then per segment frame, level, strip, x0"""
    import ctypes as C
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pbd_debug_seg_tiles
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int]
    rows = np.array([h for h, w in dims], np.int32)
    cols = np.array([w for h, w in dims], np.int32)
    cap = 1 << 16
    buf = np.zeros(16 * cap, np.int32)
    n = fn(len(dims), rows.ctypes.data_as(C.POINTER(C.c_int)), cols.ctypes.data_as(C.POINTER(C.c_int)), nb,
           buf.ctypes.data_as(C.POINTER(C.c_int)), cap)
    assert 0 <= n <= cap
    return buf[:16 * n].reshape(n, 16)


def seg_tile_counts(dims, nb):
    """what the strip-sequence tiles of nb frames of a level list hold (the kernel's own `interior` rule restated)"""
    out = dict(seg1=0, seg2=0, seg3=0, two_levels=0, three_levels=0, two_frames=0, interior=0, interior_and_border=0,
               border_tiles_with_inside_windows=0, tiles=0)
    for r in seg_tiles(dims, nb):
        ns = int(r[0])
        segs = [(int(r[1 + k]),) + tuple(int(v) for v in r[4 + 4 * k:8 + 4 * k]) for k in range(ns)]     # len, frame, level, strip, x0
        out["tiles"] += 1
        out["seg%d" % ns] += 1
        nlev = len({(s[1], s[2]) for s in segs})
        out["two_levels"] += nlev >= 2
        out["three_levels"] += nlev == 3
        out["two_frames"] += len({s[1] for s in segs}) >= 2
        inner = []
        for ln, f, l, st, x0 in segs:
            H, W = dims[l]
            inner.append(x0 >= 2 and x0 + ln + 2 <= W and 4 * st >= 2 and 4 * st + 4 + 2 <= H)
        out["interior"] += all(inner)
        out["interior_and_border"] += any(inner) and not all(inner)
        if not all(inner):       # the epilogue runs: which of its outputs take a table entry (cs != 0), which none (cs == 0)
            cs = [c31_case(4 * st + pp, x, *dims[l]) for ln, f, l, st, x0 in segs for x in range(x0, x0 + ln)
                  for pp in range(4) if 4 * st + pp < dims[l][0]]
            out["border_tiles_with_inside_windows"] += (0 in cs) and any(cs)
    return out


def mixed_plan_dims(shapes, sbin=4, interval=3):
    """pbd_debug_mixed_plan: [(frame, rows, cols)] of the virtual frame's levels of a mixed-size call"""
    import ctypes as C
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pbd_debug_mixed_plan
    fn.restype = C.c_int
    rows = np.array([s[0] for s in shapes], np.int32)
    cols = np.array([s[1] for s in shapes], np.int32)
    out = np.zeros(7 * 512, np.int32)
    n = fn(C.c_int(sbin), C.c_int(interval), C.c_int(len(shapes)), rows.ctypes.data_as(C.POINTER(C.c_int)),
           cols.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(512))
    assert 0 < n <= 512, n
    return [(int(r[0]), int(r[4]), int(r[5])) for r in out[:7 * n].reshape(n, 7)]


def plan_dims(oracle, shape, sbin=4, interval=FUSED_INTERVAL):
    """the feature-map sizes of a frame's pyramid"""
    lr, lc, _ = oracle.pyramid_plan(shape[0], shape[1], sbin, interval)
    return [tuple(int(v) for v in oracle.hog_dims(int(r), int(c), sbin)) for r, c in zip(lr, lc)]
