"""Built cases of the scale-depth pruning rule (include/pbd.h: plausible(rect, depth, fx, width, tol)).

Every case is one record in a frame of its own: a root rectangle, a hand-made depth image, the decision the rule's text gives
(`keep`, stated here, not computed by the code under test) and the branch of the rule it is built to reach (`branch`).
The images come in all four depth dtypes; what an integer dtype cannot hold (NaN, Inf, a negative, a denormal, a half-ulp
neighbour) exists for float32 / float64 only.

Parameters: fx * width / 24 = 1024 with tol = 0.25 (the band 768 .. 1280) for uint16 / float32 / float64; uint8 cannot hold
those, so its cases are the same ones at an eighth: fx * width / 24 = 128, the band 96 .. 160.
"""
from collections import namedtuple

import numpy as np

ROWS, COLS = 40, 56
RECT = (12, 8, 24, 18)              # inside the image: sample columns 16, 24, 32, sample rows 11, 17, 23
TOL = 0.25
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
BRANCHES = ("w_nonpositive", "empty_clip", "no_valid", "none_in_band", "in_band")

Case = namedtuple("Case", "name rect image keep branch")


def cfg(dtype):
    """(fx, width, tol) of the dtype's cases"""
    return (512.0, 6.0 if np.dtype(dtype) == np.uint8 else 48.0, TOL)


def levels(dtype):
    """Z for w = 24, the band's edges, and two valid values far outside the band"""
    z = 128 if np.dtype(dtype) == np.uint8 else 1024
    return dict(Z=z, LO=z * 3 // 4, HI=z * 5 // 4, FAR=z * 2 - 6, NEAR=z // 8)


def points(rect, rows=ROWS, cols=COLS):
    """the nine sample points (py, px) of the rule's step 3, row by row"""
    x, y, w, h = rect
    x1, y1, x2, y2 = max(x, 0), max(y, 0), min(x + w, cols), min(y + h, rows)
    assert x2 > x1 and y2 > y1
    return [(y1 + ((2 * j + 1) * (y2 - y1)) // 6, x1 + ((2 * i + 1) * (x2 - x1)) // 6) for j in range(3) for i in range(3)]


def image(dtype, fill, rows=ROWS, cols=COLS):
    return np.full((rows, cols), fill, dtype)


def with_samples(dtype, fill, rect, values):
    """an image of `fill` whose nine sample points of `rect` hold `values` (one value, or nine)"""
    im = image(dtype, fill)
    vals = list(values) if np.ndim(values) else [values] * 9
    for (py, px), v in zip(points(rect), vals):
        im[py, px] = v
    return im


def build(dtype):
    """the cases of one depth dtype, in a fixed order"""
    dt = np.dtype(dtype)
    L = levels(dt)
    Z, LO, HI, FAR, NEAR = L["Z"], L["LO"], L["HI"], L["FAR"], L["NEAR"]
    flt = dt.kind == "f"
    out = []

    def add(name, rect, im, keep, branch):
        assert im.dtype == dt and branch in BRANCHES
        out.append(Case(f"{dt.name}:{name}", tuple(rect), im, bool(keep), branch))

    # no valid sample: the nine points are holes, every other pixel is valid and in band -- unknown depth never prunes
    add("holes_zero", RECT, with_samples(dt, Z, RECT, 0), True, "no_valid")
    if flt:
        holes = [np.nan, np.inf, -np.inf, -0.0, -5.0, 0.0, np.nan, -np.inf, -1e-30]
        add("holes_special", RECT, with_samples(dt, Z, RECT, holes), True, "no_valid")
        tiny = np.finfo(dt).smallest_subnormal
        # a denormal is > 0: a valid sample, far out of band
        add("denormals_are_valid", RECT, with_samples(dt, Z, RECT, tiny), False, "none_in_band")
        add("one_denormal_among_holes", RECT, with_samples(dt, Z, RECT, [np.nan] * 4 + [tiny] + [0.0] * 4), False, "none_in_band")
    # valid samples, none in band: every other pixel is in band
    add("none_in_band_far", RECT, with_samples(dt, Z, RECT, FAR), False, "none_in_band")
    add("none_in_band_near", RECT, with_samples(dt, Z, RECT, NEAR), False, "none_in_band")
    add("none_in_band_mixed", RECT, with_samples(dt, Z, RECT, [FAR, NEAR, 0, FAR, NEAR, 0, FAR, NEAR, FAR]), False, "none_in_band")
    # exactly one of the nine in band, at each position in turn; the others out of band, or holes
    for k in range(9):
        add(f"one_in_band_{k}", RECT, with_samples(dt, FAR, RECT, [Z if i == k else FAR for i in range(9)]), True, "in_band")
        add(f"one_in_band_{k}_holes", RECT, with_samples(dt, FAR, RECT, [Z if i == k else 0 for i in range(9)]), True, "in_band")
    # equality on both edges
    for name, v, keep in (("lo_edge", LO, True), ("hi_edge", HI, True), ("below_lo", LO - 1, False), ("above_hi", HI + 1, False)):
        add(name, RECT, with_samples(dt, FAR, RECT, [v if i == 4 else FAR for i in range(9)]), keep, "in_band" if keep else "none_in_band")
    if flt:
        lo, hi = dt.type(LO), dt.type(HI)
        for name, v, keep in (("lo_minus_ulp", np.nextafter(lo, dt.type(0)), False), ("lo_plus_ulp", np.nextafter(lo, hi), True),
                              ("hi_minus_ulp", np.nextafter(hi, lo), True), ("hi_plus_ulp", np.nextafter(hi, dt.type(np.inf)), False)):
            add(name, RECT, with_samples(dt, FAR, RECT, [v if i == 8 else 0 for i in range(9)]), keep,
                "in_band" if keep else "none_in_band")
    # the rectangle's own width sets Z: a box twice as wide expects half the depth
    wide = (4, 4, 48, 30)
    add("wide_box_at_half_depth", wide, image(dt, Z // 2), True, "in_band")
    add("wide_box_at_full_depth", wide, image(dt, Z), False, "none_in_band")
    add("box_at_half_depth", RECT, image(dt, Z // 2), False, "none_in_band")
    # clipped on each side: Z still comes from w = 24, and the points from the clipped rectangle
    for name, rect in (("clip_left", (-10, 8, 24, 18)), ("clip_top", (12, -9, 24, 18)), ("clip_right", (COLS - 14, 8, 24, 18)),
                       ("clip_bottom", (12, ROWS - 7, 24, 18)), ("clip_corner", (-20, -15, 24, 18))):
        pts = points(rect)
        im = image(dt, FAR)
        im[pts[4]] = Z
        add(name + "_centre_in_band", rect, im, True, "in_band")
        im = image(dt, Z)
        for p in pts:
            im[p] = FAR
        add(name + "_points_out_of_band", rect, im, False, "none_in_band")
    # fully outside, on every side, and far away
    for name, rect in (("out_left", (-24, 8, 24, 18)), ("out_right", (COLS, 8, 24, 18)), ("out_top", (12, -18, 24, 18)),
                       ("out_bottom", (12, ROWS, 24, 18)), ("out_far", (1 << 30, -(1 << 30), 1 << 30, 1 << 30)),
                       ("h_zero", (12, 8, 24, 0)), ("h_negative", (12, 8, 24, -4))):
        add(name, rect, image(dt, FAR), True, "empty_clip")
    # w <= 0
    for name, rect in (("w_zero", (12, 8, 0, 18)), ("w_negative", (12, 8, -3, 18)), ("w_min", (12, 8, -(1 << 31), 18))):
        add(name, rect, image(dt, FAR), True, "w_nonpositive")
    # w = 1: Z = fx * width, which only some dtypes can hold
    zw1 = int(cfg(dt)[0] * cfg(dt)[1])
    if flt or zw1 <= np.iinfo(dt).max:
        add("w_one_in_band", (20, 10, 1, 6), image(dt, zw1), True, "in_band")
    add("w_one_out_of_band", (20, 10, 1, 6), image(dt, Z), False, "none_in_band")
    # clipped width 1 .. 7: every residue of the / 6.  The in-band value sits in the middle sample's column only; the twin puts it
    # in every column of the clipped rectangle that is NOT sampled
    for cw in range(1, 8):
        rect = (COLS - cw, 8, 24, 18)
        cols = sorted({px for _, px in points(rect)})
        im = image(dt, FAR)
        im[:, points(rect)[4][1]] = Z
        add(f"clipped_width_{cw}", rect, im, True, "in_band")
        rest = [c for c in range(COLS - cw, COLS) if c not in cols]
        if rest:
            im = image(dt, FAR)
            im[:, rest] = Z
            add(f"clipped_width_{cw}_unsampled", rect, im, False, "none_in_band")
    # a region of a larger image: rows of the parent's pitch; the parent holds the opposite answer around the region
    big = image(dt, Z, 2 * ROWS, 2 * COLS + 5)
    big[10:10 + ROWS, 20:20 + COLS] = FAR
    add("region_out_of_band", RECT, big[10:10 + ROWS, 20:20 + COLS], False, "none_in_band")
    big = image(dt, FAR, 2 * ROWS, 2 * COLS + 5)
    big[10:10 + ROWS, 20:20 + COLS] = Z
    add("region_in_band", RECT, big[10:10 + ROWS, 20:20 + COLS], True, "in_band")
    return out


def records(cases, max_parts, frame_offset=0):
    """one record per case, frame = its index + frame_offset: (n, 8 + 4 * max_parts) int32.  The other parts and header words
    hold distinct values, so that a copied record can be told from any other"""
    stride = 8 + 4 * max_parts
    rec = np.zeros((len(cases), stride), np.int32)
    for i, c in enumerate(cases):
        nparts = 1 + (i % max_parts)
        rec[i, :8] = (i + frame_offset, i % 2, i % 5, 3 + i, 4 + i, np.float32(0.25 * i - 3).view(np.int32), nparts, 0)
        rec[i, 8:12] = c.rect
        rec[i, 12:] = np.arange(stride - 12) * 7 + 1000 * i
    return rec


def bad_records(max_parts, nframes, frame_offset=0):
    """records no frame or part count of a call fits: (rows, what is wrong).  Their rectangles would be kept."""
    stride = 8 + 4 * max_parts
    rec = np.zeros((5, stride), np.int32)
    rec[:, 6] = 1
    rec[:, 8:12] = (-100, -100, 5, 5)          # fully outside: kept, were the record good
    rec[0, 0] = frame_offset - 1               # frame index -1
    rec[1, 0] = frame_offset + nframes         # one past the last frame
    rec[2, 0] = frame_offset + (1 << 30)
    rec[3, 0] = frame_offset
    rec[3, 6] = 0                              # nparts 0
    rec[4, 0] = frame_offset
    rec[4, 6] = max_parts + 1
    return rec
