"""Built hard depth images for the two stages that read one: the depth-consistency filter (pbd_kernels_consistency.hip) and the
3-D boxes (pbd_kernels_depth.hip).  Used by tests/test_depth_hard_cpu.py and tests/test_gpu_depth_hard.py.

Builders only: numpy, no handle, fixed seeds, so every machine builds the same inputs.  What each case promises is stated by
its construction (never computed from the code under test) and asserted from the yardsticks in tests/test_depth_hard_cpu.py;
DESIGN.md sections 6c and 6f, "Built hard depth images", have the tables of cases, kernels and branches.

Depth consistency: one record = a 1 x 1 parent box that holds A + a child box of M samples.  With zfactor = 0 the record is kept
exactly when the child's median (rank M // 2) equals A in T, or is not > 0.
3-D boxes: one-part records over a hole-free box, whose sorted samples are a gentle ramp with one step at rank a, so the walk from
row 200 ends next to the step's row.

The sizes named here restate constants of the kernels (partsbaseddetector_amd/csrc/pbd_internal.h, pbd_kernels_consistency.hip,
pbd_kernels_depth.hip): a case that crosses one of them says which, and tests/test_depth_hard_cpu.py reads the constexpr lines
of those files and asserts that the numbers here are theirs.
"""
from collections import namedtuple

import numpy as np

WAVE_KEYS = 1024         # kDcWaveKeys: medians of up to this many samples run on one wave
BLOCK_KEYS = 4096        # kDcBlockKeys: up to this many on one 256-thread workgroup; larger boxes stream
DC_MAX_GRID = 4096       # kDcMaxGrid: k_dc_classify makes a second grid-stride trip past DC_MAX_GRID * 256 tasks
DC_THREADS = 256         # kDcThreads: records per workgroup of k_dc_decide / k_dc_emit
# workgroups of the three select launches (launch_dc_select: kDcMaxGrid * 4, kDcMaxGrid, kDcMaxGrid / 4): a class with more
# medians than its grid makes workgroups take a second median
DC_SELECT_GRIDS = (4 * DC_MAX_GRID, DC_MAX_GRID, DC_MAX_GRID // 4)
B3_MAX_GRID = 2048       # kB3MaxGrid: longer lists make a workgroup of k_boxes3d compute a second record
B3_OUT = 400             # rows of the resample

F32, F64 = np.float32, np.float64
CODES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32, "f64": np.float64}
# flavours of a 64F image whose A is a float32 value: 'f64f' steps by float ulps on both sides; 'f64m' has distinct doubles that
# are one float below A and float-ulp neighbours above it
F64_FLOAT = ("f64f", "f64m")


def image_code(code):
    """the depth image a case of flavour `code` lives in"""
    return "f64" if code in F64_FLOAT else code


# ---- order-preserving keys (the restatement of float_key / double_key the builders step along) --------------------------------
def key_bits(code, T):
    """bits of the select's key for depth code `code` under real type T"""
    return {"u8": 8, "u16": 16, "f32": 32, "f64f": 32, "f64m": 32, "f64": 64 if T == F64 else 32}[code]


def key_of(v, code):
    """the order-preserving unsigned key of a sample of depth code `code` (a float: sign bit set for positives, all bits
    flipped for negatives); a flavour of F64_FLOAT is a double that holds a float32 value, keyed as that float"""
    if code in ("u8", "u16"):
        return int(v)
    if code == "f64":
        b = int(np.array(v, F64).view(np.uint64))
        return (~b) & (2 ** 64 - 1) if b >> 63 else b | (1 << 63)
    b = int(np.array(v, F32).view(np.uint32))
    return (~b) & (2 ** 32 - 1) if b >> 31 else b | (1 << 31)


def from_key(k, code):
    if code == "u8":
        return np.uint8(k)
    if code == "u16":
        return np.uint16(k)
    if code == "f64":
        b = k & (2 ** 63 - 1) if k >> 63 else (~k) & (2 ** 64 - 1)
        return np.array(b, np.uint64).view(F64)[()]
    b = k & (2 ** 31 - 1) if k >> 31 else (~k) & (2 ** 32 - 1)
    v = np.array(b, np.uint32).view(F32)[()]
    return F64(v) if code in F64_FLOAT else v


def _key_max(code):
    """the largest key that is a sample: the type's maximum, +Inf for floats"""
    return {"u8": 255, "u16": 65535}.get(code) or key_of(np.inf, code)


class Ladder:
    """the values around A in key order: below(j) / above(j) are j steps away (one integer, one ulp of the key's float type),
    clamped to 0 (integers) and to +Inf / the type's maximum"""

    def __init__(self, A, code):
        self.A, self.code, self.k = A, code, key_of(A, code)
        self.has_above = self.k < _key_max(code)

    def below(self, j):
        if self.code == "f64m":                                   # 4 - j double ulps above the float below A: one float, three doubles
            down = from_key(self.k - 1, "f64f")
            return from_key(key_of(down, "f64") + 4 - min(j, 3), "f64")
        return from_key(max(self.k - j, 0), self.code)

    def above(self, j):
        return from_key(min(self.k + j, _key_max(self.code)), self.code)

    def specials_below(self):
        """values below any positive A that a sign, zero or NaN slip in the key would misplace (NaN reads as 0)"""
        if self.code in ("u8", "u16"):
            return [from_key(0, self.code)]
        t = F32 if self.code != "f64" else F64
        tiny = -1e-40 if t == F32 else -1e-310                   # negative denormals
        return [t(v) for v in (-np.inf, -1e30, -3.5, tiny, -0.0, 0.0, np.nan, np.nan)]

    def specials_above(self):
        if self.code in ("u8", "u16") or not np.isfinite(self.A):
            return []
        t = F32 if self.code != "f64" else F64
        return [v for v in (t(np.inf), t(3e38)) if v > self.A]


# ---- depth consistency ---------------------------------------------------------------------------------------------------------
DcCase = namedtuple("DcCase", "name code M cls variant box parent keeps")
# box / parent: the record's child and parent part boxes (x, y, w, h), the child's possibly reaching outside the image;
# keeps: {T: promised keep bit} for the real types the case is built for

DC_W = 256                                               # width of every consistency image
# child boxes (w, h): each size class at its edges, odd and even M, widths 1, 63, 64, 65 and single rows / columns
DC_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 1), (1, 3), (63, 1), (1, 63), (64, 1), (8, 8), (65, 1), (5, 13),
             (33, 31), (64, 16), (32, 32), (41, 25),                      # 1023, 1024, 1024, 1025: the one-wave class ends
             (63, 65), (65, 63), (64, 64), (241, 17),                     # 4095, 4095, 4096, 4097: the workgroup class ends
             (70, 70), (141, 142), (100, 200)]                            # 4900, 20 022, 20 000: the streaming class
# (declared box relative to its strip, the clipped area): the image edge cuts the box, M is the clipped area
DC_CLIPPED = {"clipL": ((-7, 0, 70, 70), (63, 70)), "clipR": ((DC_W - 30, 0, 64, 20), (30, 20)), "clipB": ((0, 0, 65, 50), (65, 17))}
# A per depth code with every key byte strictly between 0x00 and 0xff, so that a decoy can replace any byte on either side
DC_A = {"u8": np.uint8(100), "u16": np.uint16(0x6A5B), "f32": F32(np.pi), "f64": F64(np.pi), "f64f": F64(F32(np.pi))}


def size_class(M):
    return 0 if M <= WAVE_KEYS else 1 if M <= BLOCK_KEYS else 2


def _as_T(v, code, T):
    """a sample as the stage reads it: integers exactly, 64F rounded to float under T = float; NaN reads as 0"""
    t = F32 if (code == "f32" or T == F32) and code not in ("u8", "u16") else F64
    with np.errstate(over="ignore", under="ignore"):
        x = t(v)
    return t(0) if np.isnan(x) else x


def promised_keep(med, A, code, T):
    """zfactor = 0: kept iff the child's median is not > 0 (no test) or equals A in T (Inf - Inf is NaN: kept)"""
    m, a = _as_T(med, code, T), _as_T(A, code, T)
    return bool(not (m > 0 and a > 0) or m == a)


def _decoy(rng, lad, side):
    """A with exactly one key byte replaced, the byte uniform over the key's bytes, the result on `side` (-1 below, +1 above) and
    not a NaN"""
    nbytes = key_bits(lad.code, F64) // 8
    while True:
        b = int(rng.integers(nbytes))
        a = (lad.k >> (8 * b)) & 255
        nv = int(rng.integers(0, a)) if side < 0 else int(rng.integers(a + 1, 256))
        v = from_key((lad.k & ~(255 << (8 * b))) | (nv << (8 * b)), lad.code)
        if not np.isnan(v):
            return v


def child_samples(rng, A, code, M, variant, mixed=True):
    """(the M samples in random order, the median by construction).  'exact': A at rank M // 2; 'below' / 'above': A one rank
    below / above it, so the median is A's neighbour one step up / down; 'decoy*': the same ranks, every other sample a decoy"""
    lad = Ladder(A, code)
    base = variant.replace("decoy-", "")
    nb = M // 2 + {"exact": 0, "below": -1, "above": 1}[base]
    if nb < 0 or nb > M - 1 or (base == "below" and not lad.has_above):
        return None
    na = M - nb - 1
    decoy = variant.startswith("decoy")

    def side(n, near, step, special, s):
        out = [near] * min(n, 1)                                  # the neighbour one step away decides an off-by-one rank
        for _ in range(n - len(out)):
            if decoy:
                out.append(_decoy(rng, lad, s))
            elif mixed and special and rng.random() < 0.3:
                out.append(special[int(rng.integers(len(special)))])
            else:
                out.append(step(int(rng.integers(1, 4))))
        return out

    lo = side(nb, lad.below(1), lad.below, lad.specials_below(), -1)
    if lad.has_above:
        hi = side(na, lad.above(1), lad.above, lad.specials_above(), +1)
    else:
        hi = [A] * na                                             # nothing above the type's maximum / +Inf: copies of A
    vals = lo + [A] + hi
    dt = CODES[image_code(code)]
    arr = np.array(vals, dt)
    rng.shuffle(arr)
    med = {"exact": A, "below": lad.above(1), "above": lad.below(1)}[base]
    return arr, med


def _dc_specs():
    """(name, code, A, (w, h) or clipped name, variants, real types, mixed) of every consistency case"""
    specs = []
    three = ("exact", "below", "above")
    for code in ("u8", "u16", "f32", "f64", "f64f"):
        A = DC_A[code]
        # 64F neighbours one double ulp apart are one float: under T = float those records keep regardless (promised_keep
        # says so); their decoys are built for T = double alone
        both = (F32, F64)
        for shape in DC_SHAPES + list(DC_CLIPPED):
            specs.append((f"{code}-A", code, A, shape, three, both, True))
        for shape in [(2, 1), (5, 13), (41, 25), (241, 17), (70, 70)]:
            specs.append((f"{code}-decoy", code, A, shape, ("decoy-exact", "decoy-below", "decoy-above"),
                          (F64,) if code == "f64" else both, False))
    edge_shapes = [(5, 13), (41, 25), (241, 17)]                 # one per size class
    for shape in [(3, 1), (64, 16)] + edge_shapes + [(70, 70)]:
        specs.append(("f64m-A", "f64m", DC_A["f64f"], shape, three, (F32, F64), True))
    f32_min, f64_min = np.array(1, np.uint32).view(F32)[()], np.array(1, np.uint64).view(F64)[()]
    edges = [("u8", np.uint8(255), "max"), ("u8", np.uint8(1), "one"), ("u16", np.uint16(65535), "max"), ("u16", np.uint16(1), "one"),
             ("f32", f32_min, "denorm"), ("f32", np.finfo(F32).max, "fltmax"), ("f32", F32(np.inf), "inf"),
             ("f64", f64_min, "denorm"), ("f64", np.finfo(F64).max, "dblmax"), ("f64", F64(np.inf), "inf"),
             ("f64f", F64(f32_min), "denorm"), ("f64f", F64(np.finfo(F32).max), "fltmax")]
    for code, A, tag in edges:
        for shape in edge_shapes:
            specs.append((f"{code}-{tag}", code, A, shape, three, (F32, F64), True))
    return specs


def _wave_rows(A, code):
    """the wave-atomic stress box, 64 x 2: a row of 64 distinct low bytes (A .. A + 63, or one step lower) next to a row of 64
    copies of A's lower neighbour: wave_add_by_key runs with 64 leaders, then with 1.  M = 128, rank 64"""
    lad = Ladder(A, code)
    dt = CODES[image_code(code)]
    out = {}
    for variant, first in (("exact", 0), ("above", -1)):         # A at rank 64, or at rank 65 (the median is its lower neighbour)
        row0 = [lad.above(first + j) if first + j > 0 else A if first + j == 0 else lad.below(1) for j in range(64)]
        out[variant] = (np.array([row0, [lad.below(1)] * 64], dt), A if variant == "exact" else lad.below(1))
    return out


def consistency_cases(seed=7):
    """{image code ('u8', 'u16', 'f32', 'f64'): (depth image, [DcCase])}.  Each case owns a strip of the image: the parent
    pixel at its top left, the child box in the rows below.  'f64f' cases (doubles that hold floats) live in the f64 image."""
    rng = np.random.default_rng(seed)
    strips = {c: [] for c in ("u8", "u16", "f32", "f64")}
    cases = {c: [] for c in strips}
    rows = {c: 0 for c in strips}

    def place(img_code, name, code, A, arr2d, decl, med, variant, reals, last=False):
        dt = CODES[img_code]
        h, w = arr2d.shape
        x_img = max(decl[0], 0)
        strip = np.zeros((1 + h, DC_W), dt)
        strip[0, 0] = A
        strip[1:, x_img:x_img + w] = arr2d
        y0 = rows[img_code]
        strips[img_code].append(strip)
        rows[img_code] += 1 + h
        box = (decl[0], y0 + 1 + decl[1], decl[2], decl[3])
        keeps = {T: promised_keep(med, A, code, T) for T in reals}
        cases[img_code].append(DcCase(f"{name}-{w}x{h}-{variant}", code, w * h, size_class(w * h), variant, box, (0, y0, 1, 1), keeps))

    deferred = []
    for name, code, A, shape, variants, reals, mixed in _dc_specs():
        img_code = image_code(code)
        if isinstance(shape, str):
            decl, (w, h) = DC_CLIPPED[shape]
        else:
            (w, h), decl = shape, (0, 0, shape[0], shape[1])
        for variant in variants:
            got = child_samples(rng, A, code, w * h, variant, mixed)
            if got is None:
                continue
            args = (img_code, name, code, A, got[0].reshape(h, w), decl, got[1], variant, reals)
            if shape == "clipB":
                deferred.append(args)                             # cut by the bottom edge: only as an image's last strip
            else:
                place(*args)
    for code in ("u8", "u16", "f32", "f64", "f64f"):
        for variant, (arr, med) in _wave_rows(DC_A[code], code).items():
            place(image_code(code), f"{code}-wave", code, DC_A[code], arr, (0, 0, 64, 2), med, variant, (F32, F64))
    # one bottom-clipped case per image, the last strip: the rest of its declared box is below the image
    seen = set()
    for args in deferred:
        if args[0] not in seen:
            seen.add(args[0])
            place(*args)
    return {c: (np.concatenate(strips[c], axis=0), cases[c]) for c in strips}


def dc_records(cases, stride, frame=0, nparts=2, component=0):
    """int32 records (n, stride) of DcCase list: part 0 the parent box, part 1 the child box; further parts far outside any image"""
    rec = np.zeros((len(cases), stride), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 6] = frame, component, nparts
    for j in range(2, nparts):
        rec[:, 8 + 4 * j:12 + 4 * j] = (-1000, -1000, 5, 5)
    for i, c in enumerate(cases):
        rec[i, 8:12] = c.parent
        rec[i, 12:16] = c.box
    return rec


def probe_cases(cases, T):
    """a short list of kept and dropped probes (one exact and one off-by-one case per size class) for the long lists"""
    out = []
    for cls in range(3):
        for keep in (True, False):
            out.append(next(c for c in cases if c.cls == cls and c.M > 3 and c.keeps.get(T) is keep and c.name.split("-")[1] == "A"))
    return out


def long_list(probes, stride, nparts, n, every=97, dense_from=None):
    """n records of an nparts-part component: a probe (cycling through `probes`) at every `every`-th position and at every
    position from `dense_from` on; all other records have every box outside the depth image (no median: kept by contract).
    Returns (records, promised keep mask from the probes' promises being filled in by the caller: the probe index per record,
    -1 for a filler)"""
    rec = np.zeros((n, stride), np.int32)
    rec[:, 6] = nparts
    rec[:, 8:8 + 4 * nparts] = np.tile(np.array([-1000, -1000, 5, 5], np.int32), nparts)
    rec[:, 2] = np.arange(n) % 1000                               # a distinguishing word, so a misplaced record shows
    rec[:, 3] = np.arange(n) // 1000
    which = np.full(n, -1, np.int64)
    k = 0
    for i in range(n):
        if i % every == 0 or (dense_from is not None and i >= dense_from):
            c = probes[k % len(probes)]
            rec[i, 8:12], rec[i, 12:16] = c.parent, c.box
            which[i] = k % len(probes)
            k += 1
    return rec, which


def emit_list(probes, T, stride, n=1500):
    """n probe records whose kept / dropped pattern has no period that divides DC_THREADS: runs of kept records straddle the
    workgroup boundaries of k_dc_emit, and workgroups hold different kept counts"""
    kept = [c for c in probes if c.keeps[T]]
    drop = [c for c in probes if not c.keeps[T]]
    rec = np.zeros((n, stride), np.int32)
    rec[:, 6] = 2
    rec[:, 2] = np.arange(n)
    pattern = np.zeros(n, bool)
    for i in range(n):
        pattern[i] = (i * i + i // 3) % 7 < 2 + (i // 200) % 4 or 250 <= i < 262 or 760 <= i < 775   # runs across records 256, 768
        c = (kept if pattern[i] else drop)[i % 3]
        rec[i, 8:12], rec[i, 12:16] = c.parent, c.box
    return rec, pattern


def reentry_list(cases, T, stride, counts=(9000, 4200, 1100)):
    """2-part records built from every case of one image, cycling through the cases of each size class: counts[k] records whose
    child box is of class k, interleaved.  With the 1 x 1 parents (class 0) each class holds more medians than its select launch has
    workgroups (DC_SELECT_GRIDS), so workgroups of all three select kernels take a second median, after a first one of other
    keys (exact, off by one, decoys, key edges).  Returns (records, promised keep mask)"""
    by_cls = [[c for c in cases if c.cls == k and T in c.keeps] for k in range(3)]
    order = np.concatenate([np.full(n, k) for k, n in enumerate(counts)])
    order = order[np.random.default_rng(23).permutation(len(order))]
    rec = np.zeros((len(order), stride), np.int32)
    rec[:, 6] = 2
    rec[:, 2] = np.arange(len(order)) % 1000
    rec[:, 3] = np.arange(len(order)) // 1000
    keep = np.zeros(len(order), bool)
    seen = [0, 0, 0]
    for i, k in enumerate(order):
        c = by_cls[k][seen[k] % len(by_cls[k])]
        seen[k] += 1
        rec[i, 8:12], rec[i, 12:16] = c.parent, c.box
        keep[i] = c.keeps[T]
    return rec, keep


# ---- 3-D boxes ---------------------------------------------------------------------------------------------------------------------
B3Case = namedtuple("B3Case", "name frame parts M kind")
# parts: the record's part boxes (x, y, w, h) in frame `frame`, whose colour frame has the depth image's shape


def ramp(kind, M):
    """the M sorted float32 samples of a gentle ramp"""
    k = np.arange(M)
    if kind == "bits":                                            # consecutive float32 bit patterns from 2.0
        return (np.uint32(0x40000000) + k.astype(np.uint32)).view(F32)
    if kind == "lin":                                             # 2 + k * 1e-4, flatter for long records so the walk still moves
        return (2 + k * min(1e-4, 0.2 / M)).astype(F32)
    if kind == "zero":                                            # through zero (never 0 itself): the key order flips at the sign
        return ((k - M // 2 + 0.5) * min(1e-4, 0.2 / M)).astype(F32)
    if kind == "denorm":                                          # denormals: |d| never passes 0.035, the walk runs to both ends
        return (np.uint32(3) + k.astype(np.uint32)).view(F32)
    raise KeyError(kind)


def stepped(kind, M, a, step):
    """ramp(kind, M) with the ranks from a upward raised by step (step > 0) or the ranks below a lowered by -step (step < 0)"""
    S = ramp(kind, M).copy()
    k = np.arange(M)
    if step > 0:
        S[k >= a] += F32(step)
    else:
        S[k < a] += F32(step)
    assert (np.diff(S) >= 0).all() and not (S == 0).any()
    return S


class _Packer:
    """shelf packing of boxes into frames of a fixed width"""

    def __init__(self, dtype, width, max_rows=400):
        self.dtype, self.width, self.max_rows = dtype, width, max_rows
        self.frames, self.cur = [], None
        self.x = self.y = self.shelf = 0

    def _new(self, rows):
        self.cur = np.full((max(rows, self.max_rows), self.width), 1, self.dtype)     # background: valid samples nobody reads
        self.frames.append(self.cur)
        self.x = self.y = self.shelf = 0

    def put(self, arr):
        h, w = arr.shape
        if self.cur is None:
            self._new(h)
        if self.x + w > self.width:
            self.x, self.y, self.shelf = 0, self.y + self.shelf, 0
        if self.y + h > self.cur.shape[0]:
            self._new(h)
        x, y = self.x, self.y
        self.cur[y:y + h, x:x + w] = arr
        self.x += w
        self.shelf = max(self.shelf, h)
        return len(self.frames) - 1, (x, y, w, h)


def _shape_of(M):
    """(w, h) with w * h = M: wide and tall boxes, widths 1 and 400+, heights below and above 16 (one wave reads one row)"""
    return {2: (2, 1), 150: (15, 10), 400: (20, 20), 401: (401, 1), 799: (17, 47), 800: (32, 25), 801: (89, 9), 1013: (1, 1013),
            4000: (125, 32), 70000: (280, 250), 1071: (63, 17), 1024: (64, 16), 975: (65, 15), 3999: (129, 31)}[M]


B3_STEPS = (1.0, 0.3, 0.2)


def _sweep_specs():
    """(M, ramp kind, step, target rows) of the float32 sweeps.  The dense M = 400 sweep visits every step position; the other
    sample counts visit a spread of rows.  The filter's 35 reflected taps keep the rows within 6 of a border out of reach of any
    single step; steps of 0.3 and 0.2 reach rows 6 to 8 (and their mirror images), a step of 1.0 only row 9"""
    specs = []
    dense = list(range(-20, 420))
    border = list(range(0, 16)) + list(range(384, 400))
    specs.append((400, "bits", 1.0, dense[::2]))
    specs.append((400, "bits", -1.0, dense[1::2]))
    specs.append((400, "lin", 0.2, dense[::10]))
    specs.append((400, "zero", -0.2, dense[2::10]))
    specs.append((400, "bits", 0.3, border + dense[3::22]))
    specs.append((400, "bits", -0.3, border + dense[7::22]))
    spread = [-3, 0, 1, 9, 57, 118, 183, 199, 200, 201, 217, 290, 342, 391, 398, 399, 403]
    for i, M in enumerate((401, 799, 800, 801, 1013, 4000, 1071, 1024, 975, 3999)):
        kind = ("bits", "lin", "zero")[i % 3]
        for j, step in enumerate((1.0, -1.0, 0.3, -0.2)):
            specs.append((M, kind, step, spread[(i + j) % 3::3]))
    specs.append((150, "bits", 1.0, list(range(0, 400, 5))))
    specs.append((150, "lin", -0.4, list(range(2, 400, 5))))
    specs.append((150, "zero", 0.3, list(range(4, 400, 10))))
    specs.append((70000, "bits", 1.0, [131]))
    return specs


def boxes3d_sweeps(seed=11):
    """float32 step-in-ramp sweeps: (depth frames, [B3Case]); every frame's colour frame has its own shape (scale 1)"""
    rng = np.random.default_rng(seed)
    pk = _Packer(F32, 420)
    cases = []
    for M, kind, step, rows in _sweep_specs():
        w, h = _shape_of(M)
        for r in rows:
            a = int(round(r * M / B3_OUT))
            S = stepped(kind, M, a, step)
            f, box = pk.put(rng.permutation(S).reshape(h, w))
            cases.append(B3Case(f"M{M}-{kind}-{step:+g}-row{r}", f, [box], M, "sweep"))
    # M = 2: both clamps, sy = -1 in the first rows; and a denormal-valued record
    for vals in ([2.0, 3.5], [-1.0, 2.0], [2.0, 2.0 + 2.0 ** -22]):
        for w, h in ((2, 1), (1, 2)):
            f, box = pk.put(np.array(vals, F32).reshape(h, w))
            cases.append(B3Case(f"M2-{vals[0]}-{w}x{h}", f, [box], 2, "tiny"))
    for M in (150, 400, 801):
        w, h = _shape_of(M)
        f, box = pk.put(rng.permutation(ramp("denorm", M)).reshape(h, w))
        cases.append(B3Case(f"M{M}-denorm", f, [box], M, "denorm"))
    # holes inside the box (0 and NaN are not samples): M is the count of the others
    for M, nh in ((400, 40), (799, 1)):
        S = stepped("bits", M, M // 3, 1.0)
        arr = np.concatenate([S, np.zeros(nh // 2 + 1, F32), np.full(nh // 2, np.nan, F32)])[:M + nh]
        f, box = pk.put(rng.permutation(arr).reshape(-1, 20))
        cases.append(B3Case(f"M{M}-holes", f, [box], M, "holes"))
    # several overlapping boxes (the overlap's samples count twice) and a non-empty boundingBoxNorm box
    for a in (300, 700, 1100):
        S = stepped("lin", 40 * 30, a, 1.0)
        f, (x, y, _, _) = pk.put(rng.permutation(S).reshape(30, 40))
        parts = [(x, y, 20, 20), (x + 10, y + 5, 20, 20), (x + 5, y + 10, 25, 15), (x + 30, y + 2, 10, 27)]
        cases.append(B3Case(f"multibox-{a}", f, parts, None, "multi"))
    # the first non-empty box all holes (the NaN box, whatever the later boxes hold), after a box outside the frame
    arr = np.full((12, 30), 2.5, F32)
    arr[:, :10] = 0
    f, (x, y, _, _) = pk.put(arr)
    cases.append(B3Case("nanbox", f, [(-50, -50, 10, 10), (x, y, 10, 12), (x + 10, y, 20, 12)], None, "nanbox"))
    cases.append(B3Case("holes-second", f, [(x + 10, y, 20, 12), (x, y, 10, 12)], None, "multi"))
    return pk.frames, cases


def boxes3d_coded(code, seed=13):
    """one sweep in another depth code: (depth frames, [B3Case]).  8U / 16U: a constant level with one step of one count (a unit
    step passes 0.035 next to it and nowhere else), ramping on beyond the step; 64F: the float ramp plus offsets that round
    away, and holes that round to 0.0f"""
    rng = np.random.default_rng(seed)
    dt = CODES[code]
    pk = _Packer(dt, 420)
    cases = []
    rows = list(range(-4, 408, 11))
    for M in (400, 801, 150):
        w, h = _shape_of(M)
        for i, r in enumerate(rows if M == 400 else rows[::6]):
            a = int(round(r * M / B3_OUT))
            k = np.arange(M)
            if code in ("u8", "u16"):
                top = 250 if code == "u8" else 60000
                if i % 2 == 0:
                    S = np.where(k < a, 100, np.minimum(101 + (k - a) // 3, top))
                else:
                    S = np.where(k >= a, 100, np.maximum(99 - (a - 1 - k) // 3, 1))
                arr = S.astype(dt)
                nh = 0
            else:
                S = stepped(("bits", "lin", "zero")[i % 3], M, a, 1.0 if i % 2 == 0 else -0.25).astype(F64)
                S = S * (1 + (k % 5 - 2) * 2.0 ** -30)            # distinct doubles that round to the float
                assert (S.astype(F32).astype(F64) != S).any()
                nh = 0 if M != 400 else 20
                arr = np.concatenate([S, np.resize(np.array([1e-50, -1e-60, 0.0, 1e-46]), nh)])
            arr = rng.permutation(arr)
            arr = arr.reshape(h, w) if nh == 0 else arr.reshape(-1, 20)
            f, box = pk.put(arr)
            cases.append(B3Case(f"{code}-M{M}-row{r}", f, [box], M, "sweep"))
    return pk.frames, cases


B3_KINDS = ("normal", "copy", "small", "nanbox", "empty", "other")


def boxes3d_long_list(device, n=2500, seed=17):
    """more than B3_MAX_GRID small records: (depth frames, [B3Case]) ordered so that records i and i + B3_MAX_GRID, which one
    workgroup computes one after the other, pair every kind with every other.  `device` adds records of another frame range
    (frame index -1 here; the device form answers six NaNs)"""
    rng = np.random.default_rng(seed)
    pk = _Packer(F32, 420)
    nk = 6 if device else 5
    regions = {}
    for kind, (w, h) in (("normal", (21, 21)), ("copy", (20, 20)), ("small", (7, 9))):
        regions[kind] = []
        for v in range(8):
            M = w * h
            S = stepped(("bits", "lin", "zero")[v % 3], M, int(M * (0.08 + 0.11 * v)), 1.0 if v % 2 else -1.0)
            regions[kind].append(pk.put(rng.permutation(S).reshape(h, w)))
    f0, hole = pk.put(np.zeros((6, 6), F32))
    assert len(pk.frames) == 1                                    # every region in one frame: a record's boxes share it
    cases = []
    for i in range(n):
        j = i - B3_MAX_GRID
        kind = B3_KINDS[i % nk if j < 0 else (j % nk + j // nk) % nk]
        if kind in regions:
            f, box = regions[kind][(i * 7) % 8]
            cases.append(B3Case(f"{i}-{kind}", f, [box], box[2] * box[3], kind))
        elif kind == "nanbox":
            f, box = regions["normal"][i % 8]
            cases.append(B3Case(f"{i}-{kind}", f0, [hole, box], None, kind))
        elif kind == "empty":
            cases.append(B3Case(f"{i}-{kind}", 0, [(-90, -90, 20, 20), (5000, 3, 4, 4)], None, kind))
        else:
            f, box = regions["copy"][i % 8]
            cases.append(B3Case(f"{i}-{kind}", -1, [box], None, kind))
    return pk.frames, cases


def b3_records(cases, stride, frame_offset=0):
    """int32 records (n, stride) of B3Case list"""
    rec = np.zeros((len(cases), stride), np.int32)
    for i, c in enumerate(cases):
        parts = np.asarray(c.parts, np.int32).reshape(-1, 4)
        rec[i, 0], rec[i, 6] = c.frame + frame_offset, len(parts)
        rec[i, 2] = i
        rec[i, 8:8 + parts.size] = parts.ravel()
    return rec
