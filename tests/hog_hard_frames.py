"""Frames that drive the resampling and HOG kernels (csrc/pbd_kernels_features.hip; src/HOGFeatures.cpp:99-341) into the cases
ordinary scenes barely reach -- saturated gradients, the rounding edges of the fixed-point resize and pyrDown, the exact ties of
the orientation snap and of the strongest-channel pick, pixels next to a bisector of two orientations -- and plain float64 /
integer statements of the operations themselves.  Shared by tests/test_gpu_feature_variants.py (every kernel variant against the
oracle, bit for bit) and tests/test_oracle_cpu.py (the oracle against these references, on the same frames).

Everything is seeded through synth's counter-based generator and built with integer or exactly representable arithmetic, so
the same call gives the same bytes on every machine.  Frames are at most 200 x 200."""
import itertools

import numpy as np

from partsbaseddetector_amd import synth

SBINS = (2, 3, 4, 5, 6, 8)
UU = np.array([1.000, 0.9397, 0.7660, 0.5000, 0.1736, -0.1736, -0.5000, -0.7660, -0.9397])
VV = np.array([0.000, 0.3420, 0.6428, 0.8660, 0.9848, 0.9848, 0.8660, 0.6428, 0.3420])


def hwc(im):
    im = np.asarray(im)
    return im if im.ndim == 3 else im[:, :, None]


# ---- the references -------------------------------------------------------------------------------------------------------------
def snap_f64(dx, dy):
    """The 18-way orientation snap (src/HOGFeatures.cpp:236-250) in float64 on arrays of gradients: the chosen bin (the scan
    keeps the first of equal maxima: strict `>`, k ascending, dot before -dot), the best dot product and its margin over the
    second-best of the 18 signed dot products."""
    dots = UU.reshape((9,) + (1,) * np.ndim(dx)) * dx + VV.reshape((9,) + (1,) * np.ndim(dx)) * dy
    k = np.argmax(np.abs(dots), axis=0)                                  # first k of equal |dot|
    d = np.take_along_axis(dots, k[None], axis=0)[0]
    ori = np.where(d < 0, k + 9, k)
    ori = np.where(d == 0, 0, ori)                                       # nothing beats the initial best = 0
    both = np.sort(np.concatenate([dots, -dots], axis=0), axis=0)
    return ori, both[-1], both[-1] - both[-2]


def hog_reference_f64(im, sbin):
    """HOG features of one image (matlab/mex/features.cc as adapted by src/HOGFeatures.cpp:168-341) in float64, scatter form,
    vectorised: independent of the oracle's and the kernels' code.  Any sbin >= 2, any accepted pixel type; the differences are
    taken in the pixel type (an integer difference for uint8 / uint16, `a - b` in float32 / float64) and then widened.

    Returns (feat (out_rows, out_cols * 32), margin (blk_rows, blk_cols)): margin[by, bx] is the smallest RELATIVE float64
    margin (best minus second-best signed dot product, over the best) of the pixels that feed block (by, bx); inf where none do."""
    im = hwc(im)
    rows, cols, cn = im.shape
    bh, bw = int(np.floor(rows / sbin + 0.5)), int(np.floor(cols / sbin + 0.5))
    oh, ow = max(bh - 2, 0), max(bw - 2, 0)
    margin = np.full((bh, bw), np.inf)
    if oh == 0 or ow == 0:
        return np.zeros((oh, ow * 32)), margin
    y = np.arange(1, bh * sbin - 1)
    x = np.arange(1, bw * sbin - 1)
    ys, xs = np.minimum(y, rows - 2), np.minimum(x, cols - 2)
    a = im.astype(np.int64) if im.dtype.kind in "ui" else im
    dy = (a[ys + 1][:, xs] - a[ys - 1][:, xs]).astype(np.float64)        # (Y, X, cn)
    dx = (a[ys][:, xs + 1] - a[ys][:, xs - 1]).astype(np.float64)
    v = dx * dx + dy * dy
    if cn == 3:                            # start from channel 2, take 1 and then 0 only on strictly larger magnitude
        c = np.full(v.shape[:2], 2)
        c = np.where(v[:, :, 1] > v[:, :, 2], 1, c)
        vc = np.take_along_axis(v, c[:, :, None], axis=2)[:, :, 0]
        c = np.where(v[:, :, 0] > vc, 0, c)
    else:
        c = np.zeros(v.shape[:2], np.int64)
    dxc = np.take_along_axis(dx, c[:, :, None], axis=2)[:, :, 0]
    dyc = np.take_along_axis(dy, c[:, :, None], axis=2)[:, :, 0]
    mag = np.sqrt(np.take_along_axis(v, c[:, :, None], axis=2)[:, :, 0])
    ori, best, gap = snap_f64(dxc, dyc)
    # dx == 0 is no near-tie: vv[4] == vv[5] and uu[4] == -uu[5] make the two dot products the same number in every precision,
    # and every arithmetic keeps the first; what could flip is the runner-up after them
    gap = np.where(dxc == 0, (VV[4] - VV[3]) * np.abs(dyc), gap)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(best > 0, gap / best, np.inf)
    yp, xp = (y + 0.5) / sbin - 0.5, (x + 0.5) / sbin - 0.5
    iy, ix = np.floor(yp).astype(np.int64), np.floor(xp).astype(np.int64)
    vy0, vx0 = yp - iy, xp - ix
    hist = np.zeros(bh * bw * 18)
    for yy, wy in ((iy, 1 - vy0), (iy + 1, vy0)):
        for xx, wx in ((ix, 1 - vx0), (ix + 1, vx0)):
            ok = ((yy >= 0) & (yy < bh))[:, None] & ((xx >= 0) & (xx < bw))[None, :]
            cell = yy[:, None] * bw + xx[None, :]
            np.add.at(hist, (cell * 18 + ori)[ok], ((wy[:, None] * wx[None, :]) * mag)[ok])
            np.minimum.at(margin.reshape(-1), cell[ok], rel[ok])
    hist = hist.reshape(bh, bw, 18)
    norm = ((hist[:, :, :9] + hist[:, :, 9:]) ** 2).sum(axis=2)
    s = norm[:-1, :-1] + norm[:-1, 1:] + norm[1:, :-1] + norm[1:, 1:]
    n = 1.0 / np.sqrt(s + 1e-4)
    ns = (n[1:, 1:], n[:-1, 1:], n[1:, :-1], n[:-1, :-1])                # cells (y+1,x+1), (y,x+1), (y+1,x), (y,x) of out (y, x)
    ns = [q[:oh, :ow, None] for q in ns]
    h = hist[1:1 + oh, 1:1 + ow]
    hs = [np.minimum(h * q, 0.2) for q in ns]
    feat = np.zeros((oh, ow, 32))
    feat[:, :, :18] = 0.5 * (hs[0] + hs[1] + hs[2] + hs[3])
    su = h[:, :, :9] + h[:, :, 9:]
    ss = [np.minimum(su * q, 0.2) for q in ns]
    feat[:, :, 18:27] = 0.5 * (ss[0] + ss[1] + ss[2] + ss[3])
    for i in range(4):
        feat[:, :, 27 + i] = 0.2357 * hs[i].sum(axis=2)
    return feat.reshape(oh, ow * 32), margin


def cells_fed_by(margin, below):
    """(out_rows, out_cols) mask of the feature cells that depend on a block whose margin is under `below`: a cell reads its own
    block's histogram and the energies of the 3 x 3 blocks around it."""
    bad = margin < below
    bh, bw = bad.shape
    out = np.zeros((max(bh - 2, 0), max(bw - 2, 0)), bool)
    for i in range(3):
        for j in range(3):
            out |= bad[i:i + bh - 2, j:j + bw - 2]
    return out


def resize_coef(dn, sn):
    """The half-pixel centre rule of INTER_LINEAR: per destination index the two source indices and the
    float fraction f of the second one (the coordinate is rounded to float before it is split, as the library does)."""
    scale = 1.0 / (float(dn) / float(sn))
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s0 = np.floor(f).astype(np.int64)
    f = (f - s0.astype(np.float32)).astype(np.float32)
    lo, hi = s0 < 0, s0 >= sn - 1
    f = np.where(lo | hi, np.float32(0), f)
    s0 = np.where(lo, 0, np.where(hi, sn - 1, s0))
    return s0, np.minimum(s0 + 1, sn - 1), f


def resize_u8_reference(im, dh, dw):
    """SURVEY Appendix E's 8-bit INTER_LINEAR algorithm written again, vectorised and from the text alone (fixed point, 11
    coefficient bits, horizontal pass in int, vertical pass ((b * (r >> 4)) >> 16 twice) + 2 >> 2) -- an independent statement
    of the same published algorithm, not a second opinion on OpenCV itself (which nothing here can provide)."""
    im = hwc(im)
    sh, sw = im.shape[:2]
    if (dh, dw) == (sh, sw):
        return im.copy()

    def fixed(dn, sn):
        s0, s1, f = resize_coef(dn, sn)
        a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)      # cvRound: half to even, as np.rint
        a1 = np.rint(f * np.float32(2048)).astype(np.int64)
        return s0, s1, a0, a1

    sx0, sx1, a0, a1 = fixed(dw, sw)
    sy0, sy1, b0, b1 = fixed(dh, sh)
    S = im.astype(np.int64)
    R = S[:, sx0] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]              # every source row, horizontally
    r0, r1 = R[sy0], R[sy1]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def resize_linear_reference(im, dh, dw):
    """Bilinear interpolation with the half-pixel centre rule in float64, for the depths that keep float coefficients (16U,
    32F, 64F): dst = (1-fy) * ((1-fx) * S00 + fx * S01) + fy * ((1-fx) * S10 + fx * S11) with resize_coef's fractions, the
    coefficient pair being the floats (1 - f, f) as in the 8-bit form, and no fixed point: sums and products in float64.  16U: round half to even, saturate.  32F / 64F: the float64 value (the caller compares with a tolerance)."""
    im = hwc(im)
    sh, sw = im.shape[:2]
    sx0, sx1, fx = resize_coef(dw, sw)
    sy0, sy1, fy = resize_coef(dh, sh)
    ax0, ax1 = (np.float32(1) - fx).astype(np.float64)[None, :, None], fx.astype(np.float64)[None, :, None]
    ay0, ay1 = (np.float32(1) - fy).astype(np.float64)[:, None, None], fy.astype(np.float64)[:, None, None]
    S = im.astype(np.float64)
    R = ax0 * S[:, sx0] + ax1 * S[:, sx1]
    out = ay0 * R[sy0] + ay1 * R[sy1]
    if im.dtype == np.uint16:
        return np.clip(np.rint(out), 0, 65535).astype(np.uint16)
    return out


def pyrdown_reference(im):
    """cv::pyrDown in its padded form: [1 4 6 4 1] x [1 4 6 4 1] over a BORDER_REFLECT_101 padding, every second pixel.
    Integer pixels: int64 sum, (sum + 128) >> 8, exact.  Float pixels: float64 sum / 256."""
    im = hwc(im)
    r, c, cn = im.shape
    integer = im.dtype.kind == "u"

    def refl(p, n):
        if n == 1:
            return np.zeros_like(p)
        p = np.abs(p)
        while (p >= n).any():
            p = np.where(p >= n, np.abs(2 * n - 2 - p), p)
        return p

    dr, dc = (r + 1) // 2, (c + 1) // 2
    k = (1, 4, 6, 4, 1)
    S = im.astype(np.int64 if integer else np.float64)
    acc = np.zeros((dr, dc, cn), S.dtype)
    for i in range(5):
        yy = refl(2 * np.arange(dr) - 2 + i, r)
        for j in range(5):
            xx = refl(2 * np.arange(dc) - 2 + j, c)
            acc += (k[i] * k[j]) * S[yy][:, xx]
    return ((acc + 128) >> 8).astype(im.dtype) if integer else acc / 256.0


# ---- 8-bit frames ---------------------------------------------------------------------------------------------------------------
def scene(seed, rows, cols, cn):
    return hwc(synth.synthetic_frame(seed, rows, cols, cn))


def noise(seed, rows, cols, cn):
    return hwc(synth.synthetic_frame(seed, rows, cols, cn, kind="noise"))


def extremes(rows, cols, cn):
    """0 / 255 only: a checkerboard (left third), one-pixel dark lines on white (middle), two-pixel bright lines on black
    (right).  Gradients saturate to +-255, the pyrDown sums sit at (v + 128) >> 8's extremes and the fixed-point resize chain
    (>> 4, >> 16, + 2 >> 2) at its rounding edges; the flat areas next to the lines give zero gradients beside saturated ones."""
    y, x = np.mgrid[0:rows, 0:cols]
    out = np.zeros((rows, cols, cn), np.uint8)
    a, b = cols // 3, 2 * cols // 3
    for c in range(cn):
        yy, xx = y + c, x + 2 * c                                        # the channels disagree about where the lines are
        board = ((yy + xx) & 1) * 255
        thin = np.where((xx % 7 == 0) | (yy % 11 == 0), 0, 255)
        thick = np.where((xx % 9 < 2) | (yy % 13 < 2), 255, 0)
        out[:, :, c] = np.where(x < a, board, np.where(x < b, thin, thick))
    return out


def vertical(seed, rows, cols, cn):
    """Rows of constant value -- stripes one, two and three pixels high, ramps of several slopes -- so that dx == 0 and dy != 0:
    uu[4]*dx + vv[4]*dy == uu[5]*dx + vv[5]*dy exactly (vv[4] == vv[5]), the only exact tie of the snap for integer gradients;
    the strict `>` keeps orientation 4 (13 for dy < 0).  The last fifth of the columns is noise, so dx != 0 occurs too."""
    y = np.arange(rows)
    out = np.zeros((rows, cols, cn), np.uint8)
    for c in range(cn):
        yy = y + 3 * c
        period = 1 + (yy // 12) % 3
        stripes = ((yy // period) & 1) * (255 - 40 * ((yy // 36) % 3))
        ramp = (yy * (1 + 2 * c + (yy // 20) % 5) * 3) % 256
        col = np.where(y < rows // 2, stripes, ramp)
        out[:, :, c] = col[:, None]
    k = cols - cols // 5
    out[:, k:] = noise(seed, rows, cols, cn)[:, k:]
    return out


def _crosses(rows, cols, cn, grads, pitch=6):
    """One 3 x 3 cross per entry of `grads` ((dx, dy) per channel, |.| <= 255) on a black frame, `pitch` pixels apart so that
    they do not interact: left / right / down / up neighbours of the centre are set so that the centre's gradient of channel
    c is exactly grads[i][c].  Entries beyond the frame's capacity are left out; returns the frame and the number placed."""
    out = np.zeros((rows, cols, cn), np.uint8)
    per_row = (cols - 3) // pitch
    n = min(len(grads), per_row * ((rows - 3) // pitch))
    for i in range(n):
        cy, cx = 2 + pitch * (i // per_row), 2 + pitch * (i % per_row)
        for c in range(cn):
            dx, dy = grads[i][c]
            out[cy, cx + 1, c], out[cy, cx - 1, c] = max(dx, 0), max(-dx, 0)
            out[cy + 1, cx, c], out[cy - 1, cx, c] = max(dy, 0), max(-dy, 0)
    return out, n


_TIE_FAMILY = [(3, 4), (5, 0), (0, 5), (-4, 3), (4, 3), (-3, 4), (3, -4), (-5, 0), (0, -5), (4, -3), (-3, -4), (-4, -3)]


def channel_tie_gradients():
    """Per cross, three channel gradients of equal squared magnitude 25 k^2 and different directions ((3,4), (5,0), (0,5),
    (-4,3), ... scaled by k = 1 .. 51), each triple in all six channel orders; every third triple has one member one step
    weaker, so that two channels tie above a third.  Rule: channel 2 unless 1 is strictly larger, then 0 only if strictly
    larger than that."""
    grads = []
    for t in range(64):
        k = 1 + (t * 7) % 51
        trio = [_TIE_FAMILY[(t + j * (1 + t % 3)) % 12] for j in range(3)]
        trio = [(k * dx, k * dy) for dx, dy in trio]
        if t % 3 == 2 and k > 1:
            dx, dy = _TIE_FAMILY[(t + 5) % 12]
            trio[t % 2] = ((k - 1) * dx, (k - 1) * dy)
        grads += [list(p) for p in itertools.permutations(trio)]
    return grads


def channel_ties(rows, cols):
    return _crosses(rows, cols, 3, channel_tie_gradients())[0]          # 384 crosses; a small frame holds the first of them


_NEAR = None


def near_bisector_pairs():
    """All (dx, dy), |dx|, |dy| <= 255 (not both 0), ordered by the relative float64 margin of the snap, smallest first: the
    511 - 1 exact ties dx == 0 lead, the pairs next to a bisector of two orientations follow."""
    global _NEAR
    if _NEAR is None:
        dy, dx = np.mgrid[-255:256, -255:256]
        dx, dy = dx.ravel(), dy.ravel()
        keep = (dx != 0) | (dy != 0)
        dx, dy = dx[keep], dy[keep]
        _, best, gap = snap_f64(dx.astype(np.float64), dy.astype(np.float64))
        order = np.argsort(gap / best, kind="stable")
        _NEAR = np.stack([dx[order], dy[order]], axis=1)
    return _NEAR


def near_bisector(rows, cols, cn, part=0):
    """Crosses for the pairs of near_bisector_pairs(), as many as the frame holds, starting at part * that many; a colour frame
    carries the pair in channel i % 3 of cross i and nothing in the others."""
    per = ((cols - 3) // 6) * ((rows - 3) // 6)
    pairs = near_bisector_pairs()[part * per:(part + 1) * per]
    grads = [[(int(dx), int(dy)) if c == i % cn else (0, 0) for c in range(cn)] for i, (dx, dy) in enumerate(pairs)]
    out, n = _crosses(rows, cols, cn, grads)
    assert n == per
    return out


def frames_u8(seed, rows, cols, cn):
    """name -> uint8 frame (rows, cols, cn): every 8-bit kind above (channel_ties for colour only)."""
    out = {"scene": scene(seed, rows, cols, cn), "noise": noise(seed + 1, rows, cols, cn), "extremes": extremes(rows, cols, cn),
           "vertical": vertical(seed + 2, rows, cols, cn), "near_bisector": near_bisector(rows, cols, cn)}
    if cn == 3:
        out["channel_ties"] = channel_ties(rows, cols)
    return out


# ---- typed frames ---------------------------------------------------------------------------------------------------------------
def _unit(seed, rows, cols, cn, stream):
    """uniform multiples of 2^-20 in [0, 1), exact in float32"""
    return ((synth.uniform_u32(seed, rows * cols * cn, stream=stream) >> 12).astype(np.float64) / float(1 << 20)).reshape(rows, cols, cn)


def frames_genuine(dtype, seed, rows, cols, cn):
    """name -> frame of `dtype` whose values use the type's own range: gradients that are no 8-bit integers.
    uint16: a scene scaled to 0 .. 65535 with 8 low bits of noise and patches of 0 and 65535.
    float32 / float64: "unit", a scene in [0, 1] with 1e-3 of noise; "wide", a scene in [-1e3, 1e3] with noise of 1.
    float64 also: "texture", an 8-bit scene plus multiples of 2^-30 that float32 cannot hold next to a value >= 1, so that a
    float intermediate anywhere in a double kernel changes the result's bits."""
    dtype = np.dtype(dtype)
    base = scene(seed, rows, cols, cn).astype(np.float64)
    if dtype == np.uint16:
        im = base.astype(np.int64) * 257 + (synth.uniform_u32(seed, rows * cols * cn, stream=21) & 0xFF).reshape(rows, cols, cn) - 128
        im[rows // 5:rows // 5 + 9, cols // 4:cols // 4 + 14] = 65535
        im[rows // 2:rows // 2 + 7, cols // 2:cols // 2 + 11] = 0
        return {"full": np.clip(im, 0, 65535).astype(np.uint16)}
    out = {"unit": (base / 255.0 + _unit(seed, rows, cols, cn, 22) * 1e-3).astype(dtype),
           "wide": ((base - 127.5) * (1e3 / 127.5) + (_unit(seed, rows, cols, cn, 23) - 0.5)).astype(dtype)}
    if dtype == np.float64:
        tex = (1 + (synth.uniform_u32(seed, rows * cols * cn, stream=24) % 1023)).reshape(rows, cols, cn)
        out["texture"] = base + tex.astype(np.float64) * 2.0 ** -30
        assert not np.array_equal(out["texture"].astype(np.float32).astype(np.float64), out["texture"])
    return out
