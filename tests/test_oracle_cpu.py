"""CPU tests of the oracle (the checker) against INDEPENDENT formulations of each stage.

The reference ships no golden vectors for this path and cannot be built here (SURVEY.md section 4 /
8c: "parity unpinned"), so the restatement is cross-checked by code with a different structure:
brute-force max-plus distance transform, scipy correlation, a scatter-form float64 HOG, an integer
numpy pyrDown, and a brute-force tree max-sum for the dynamic program.  The HOG and resampling references and
the frames they are run on live in tests/hog_hard_frames.py, shared with the GPU tests of the same kernels."""
import numpy as np
import pytest
from scipy import signal

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import synth

import dt_hard_planes as H
import hog_hard_frames as F


# ---------------------------------------------------------------------------------- geometry
def test_pyramid_plan_matches_survey_appendix_b(oracle):
    # SURVEY.md Appendix B (computed from src/HOGFeatures.cpp:99,116-124,174-175)
    for (rows, cols, interval), (levels, pixels, cells) in {
        (480, 640, 10): (46, 2371512, 140725),
        (1080, 1920, 10): (58, 16019919, 980592),
        (240, 320, 5): (18, 315695, 17945),
        (240, 320, 10): (36, 590699, 33459),
    }.items():
        lr, lc, sc = oracle.pyramid_plan(rows, cols, 4, interval)
        assert len(lr) == levels
        assert int(np.sum(lr.astype(np.int64) * lc)) == pixels
        assert sum(int(np.prod(oracle.hog_dims(int(a), int(b), 4))) for a, b in zip(lr, lc)) == cells
    lr, lc, sc = oracle.pyramid_plan(480, 640, 4, 10)
    assert (lr[0], lc[0], lr[1], lc[1], lr[2], lc[2]) == (480, 640, 448, 597, 418, 557)
    assert (lr[-1], lc[-1]) == (22, 29) and oracle.hog_dims(22, 29, 4) == (4, 5)
    assert sc[0] == 4.0 and sc[10] == 8.0 and np.all(sc[10:20] == 2 * sc[:10])


def test_plan_float_vs_double_sfactor_agree():
    # include/HOGFeatures.hpp:78: pow(2.0f, 1.0f/interval) -- float or double overload gives the same float
    for interval in (1, 2, 3, 5, 8, 10):
        a = np.float32(2.0) ** np.float32(np.float32(1.0) / np.float32(interval))
        b = np.float32(2.0 ** float(np.float32(1.0) / np.float32(interval)))
        assert np.float32(a) == b


# ---------------------------------------------------------------------------------- resampling
def test_resize_identity_and_bilinear(oracle):
    im = synth.synthetic_frame(4, 61, 83, 3)
    assert np.array_equal(oracle.resize_linear_u8(im, 61, 83), im)
    out = oracle.resize_linear_u8(im, 44, 59)
    # float64 bilinear with the same half-pixel mapping; the fixed-point path is within 1 grey level
    ys = (np.arange(44) + 0.5) * (61 / 44) - 0.5
    xs = (np.arange(59) + 0.5) * (83 / 59) - 0.5
    y0 = np.floor(ys).astype(int); fy = ys - y0
    x0 = np.floor(xs).astype(int); fx = xs - x0
    y0c, y1c = np.clip(y0, 0, 60), np.clip(y0 + 1, 0, 60)
    x0c, x1c = np.clip(x0, 0, 82), np.clip(x0 + 1, 0, 82)
    f = im.astype(np.float64)
    ref = ((1 - fy)[:, None, None] * ((1 - fx)[None, :, None] * f[y0c][:, x0c] + fx[None, :, None] * f[y0c][:, x1c])
           + fy[:, None, None] * ((1 - fx)[None, :, None] * f[y1c][:, x0c] + fx[None, :, None] * f[y1c][:, x1c]))
    assert np.abs(out.astype(np.float64) - ref).max() <= 1.01


@pytest.mark.parametrize("shape,dst", [((61, 83), (44, 59)), ((61, 83), (58, 80)), ((97, 131), (49, 66)), ((240, 320), (224, 299)),
                                       ((50, 61), (37, 45))])
@pytest.mark.parametrize("cn", [3, 1])
def test_resize_u8_against_an_independent_integer_formulation(oracle, shape, dst, cn):
    im = synth.synthetic_frame(9, shape[0], shape[1], cn)
    if im.ndim == 2:
        im = im[:, :, None]
    got = oracle.resize_linear_u8(im if cn == 3 else im[:, :, 0], dst[0], dst[1])
    want = F.resize_u8_reference(im, dst[0], dst[1])
    assert np.array_equal(np.asarray(got).reshape(want.shape), want)


def test_pyrdown_integer_formulation(oracle):
    for shape, cn in [((37, 52), 3), ((40, 41), 1), ((5, 4), 3)]:
        im = synth.synthetic_frame(9, shape[0], shape[1], cn, kind="noise")
        got = oracle.pyrdown_u8(im)
        assert np.array_equal(got, F.pyrdown_reference(im))        # the padded form, tests/hog_hard_frames.py


# ---------------------------------------------------------------------------------- HOG
@pytest.mark.parametrize("shape,cn", [((50, 61), 3), ((47, 38), 1)])
def test_hog_against_scatter_form(oracle, shape, cn):
    im = synth.synthetic_frame(2, shape[0], shape[1], cn)
    got = oracle.hog_features(im, 4)
    ref, _ = F.hog_reference_f64(im, 4)
    assert got.shape == ref.shape
    assert np.abs(got.astype(np.float64) - ref).max() < 2e-5
    assert not got.reshape(got.shape[0], -1, 32)[:, :, 31].any()        # truncation channel is 0 (:338)
    got64 = oracle.hog_features(im, 4, dtype=np.float64)
    assert np.abs(got64 - ref).max() < 1e-9


def test_hog_constant_image_is_zero(oracle):
    im = synth.synthetic_frame(0, 40, 44, 3, kind="constant")
    assert not oracle.hog_features(im, 4).any()


# ---------------------------------------------------------------------------------- convolution
def test_conv_against_scipy(oracle):
    rng = np.random.default_rng(1)
    H, W, k = 13, 17, 5
    feat = rng.random((H, W, 32)).astype(np.float32)
    feat[:, :, 31] = 0
    filt = (rng.standard_normal((k, k, 32)) * 0.1).astype(np.float32)
    filt[0, 0, 3] = 0.0   # a skipped tap
    got = oracle.conv(feat.reshape(H, W * 32), filt.reshape(k, k * 32))
    ref = np.zeros((H, W))
    for c in range(32):
        border = 1.0 if c == 31 else 0.0
        plane = np.pad(feat[:, :, c].astype(np.float64), 2, constant_values=border)
        ref += signal.correlate2d(plane, filt[:, :, c].astype(np.float64), mode="valid")
    assert np.abs(got - ref).max() < 1e-5
    # the border-of-ones: with zero features only channel 31's out-of-image taps contribute
    z = np.zeros((H, W * 32), np.float32)
    got0 = oracle.conv(z, filt.reshape(k, k * 32))
    ref0 = signal.correlate2d(np.pad(np.zeros((H, W)), 2, constant_values=1.0), filt[:, :, 31].astype(np.float64), mode="valid")
    assert np.abs(got0 - ref0).max() < 1e-6 and got0[H // 2, W // 2] == 0.0


def test_conv_even_kernel_anchor(oracle):
    rng = np.random.default_rng(2)
    feat = rng.random((6, 7, 32)).astype(np.float32)
    filt = rng.standard_normal((4, 4, 32)).astype(np.float32)
    got = oracle.conv(feat.reshape(6, 7 * 32), filt.reshape(4, 4 * 32))
    ref = np.zeros((6, 7))
    for c in range(32):
        plane = np.pad(feat[:, :, c].astype(np.float64), ((2, 1), (2, 1)), constant_values=1.0 if c == 31 else 0.0)   # anchor = k/2 = 2
        ref += signal.correlate2d(plane, filt[:, :, c].astype(np.float64), mode="valid")
    assert np.abs(got - ref).max() < 1e-4


# ---------------------------------------------------------------------------------- distance transform
def _dt_brute(score, ax, bx, ay, by, osx, osy):
    M_, N_ = score.shape
    s = score.astype(np.float64)
    n = np.arange(N_)
    dx = osx + n[:, None] - n[None, :]                    # [out n, src n']
    rows = (ax * dx * dx + bx * dx)[None, :, :] + s[:, None, :]   # [m, n, n']
    tmp = rows.max(axis=2)
    ixr = rows.argmax(axis=2)
    tmp32 = tmp.astype(np.float32).astype(np.float64)   # the reference stores the row pass in T
    m = np.arange(M_)
    dy = osy + m[:, None] - m[None, :]
    cols = (ay * dy * dy + by * dy)[:, :, None] + tmp32[None, :, :]   # [m, m', n]
    out = cols.max(axis=1)
    iyr = cols.argmax(axis=1)
    return out, ixr, iyr


@pytest.mark.parametrize("seed,shape,w,os", [(0, (9, 11), (0.01, 0.0, 0.01, 0.0), (0, 0)),
                                              (1, (23, 31), (0.01, 0.0, 0.01, 0.0), (3, -2)),
                                              (2, (17, 40), (0.012, 0.004, 0.02, -0.007), (-4, 4)),
                                              (3, (1, 25), (0.05, 0.0, 0.05, 0.0), (2, 0)),
                                              (4, (30, 1), (0.05, 0.01, 0.03, 0.0), (0, -3))])
def test_dt_against_brute_force(oracle, seed, shape, w, os):
    rng = np.random.default_rng(seed)
    score = rng.standard_normal(shape).astype(np.float32)
    ax, bx, ay, by = (-np.float32(w[0]), -np.float32(w[1]), -np.float32(w[2]), -np.float32(w[3]))
    out, Ix, Iy = oracle.dt(score, float(ax), float(bx), float(ay), float(by), os[0], os[1])
    ref, ixr, iyr = _dt_brute(score, float(ax), float(bx), float(ay), float(by), os[0], os[1])
    # scores: exact max (0 mismatches vs O(N^2) brute force)
    assert np.abs(out.astype(np.float64) - ref).max() < 2e-6
    assert np.mean(out == ref.astype(np.float32)) > 0.995
    # pointers follow the reference's composition Iy[m][n] = IyRaw[m][Ix[m][n]] (DistanceTransform.hpp:233-244)
    agree_x = np.mean(Ix == ixr)
    assert agree_x > 0.98          # envelope vs double brute force may differ on near ties
    quirk = np.take_along_axis(iyr, Ix, axis=1)
    assert np.mean(Iy == quirk) > 0.98
    assert Ix.min() >= 0 and Ix.max() < shape[1] and Iy.min() >= 0 and Iy.max() < shape[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["constant", "quantised", "spikes"])
@pytest.mark.parametrize("shape,w,os", [((9, 40), (0.25, 0.0, 0.015625, 0.0), (0, 0)),
                                        ((33, 17), (0.015625, 0.5, 0.25, 0.0), (3, -2)),
                                        ((3, 300), (0.0625, -0.25, 0.0625, 0.125), (-4, 1)),
                                        ((70, 2), (0.25, 0.0, 0.0625, -0.5), (1, 4)),
                                        ((1, 65), (0.015625, 0.0, 0.015625, 0.0), (2, 0))])
def test_dt_exact_on_hard_planes(oracle, kind, shape, w, os, dtype):
    """The planes that drive the GPU transforms into deep envelopes, long pop runs and exact ties (tests/dt_hard_planes.py), with
    power-of-two coefficients: every intermediate value is exact, so the oracle's transform equals the O(N^2) maximum bit for
    bit, and each pointer attains it -- the row pointer the row maximum, the column pointer (IyRaw[m][Ix[m][n]], the reference's
    composition) the maximum of the column it was read from.  Which of several equal maxima is returned is the envelope's
    choice, so the indices are not compared with the brute force's argmax."""
    rng = np.random.default_rng(len(kind) * 7 + shape[0])
    score = (H.plane(kind, rng, *shape) if kind != "quantised" else rng.integers(-3, 4, shape) * 0.25).astype(dtype)
    ax, bx, ay, by = (-float(np.float32(v)) for v in w)
    out, Ix, Iy = oracle.dt(score, ax, bx, ay, by, os[0], os[1])
    ref, _, _ = _dt_brute(score, ax, bx, ay, by, os[0], os[1])
    assert np.array_equal(out, ref.astype(dtype))
    M_, N_ = shape
    m, n = np.mgrid[0:M_, 0:N_]
    dx = (os[0] + n - Ix).astype(np.float64)
    row_at_ptr = ax * dx * dx + bx * dx + score.astype(np.float64)[m, Ix]
    row_max = (ax * (os[0] + n[:, :, None] - np.arange(N_)) ** 2 + bx * (os[0] + n[:, :, None] - np.arange(N_))
               + score.astype(np.float64)[:, None, :]).max(axis=2)
    assert np.array_equal(row_at_ptr, row_max)
    dy = (os[1] + m - Iy).astype(np.float64)
    col_at_ptr = ay * dy * dy + by * dy + row_max[Iy, Ix]                 # column Ix[m][n], source row Iy[m][n]
    assert np.array_equal(col_at_ptr, ref[m, Ix])                         # the maximum of that column at output row m
    _, ptr, st = H.replay_rows(score, ax, bx, os[0], dtype)
    assert np.array_equal(ptr, Ix)                                        # the replay the GPU tests measure with is computeRow


def test_hard_planes_reach_deep_envelopes_and_ties(oracle):
    """The replay's statistics on the planes the GPU tests use: constant rows keep every element (depth = N), spikes pop more
    than a cooperative window at once, quantised planes with a power-of-two quadratic tie exactly in both comparisons."""
    rng = np.random.default_rng(4)
    _, _, st = H.replay_rows(H.plane("constant", rng, 2, 600), -0.01, -0.0, 0)
    assert st["depth"].min() == 600 and st["maxpop"].max() == 0
    _, _, st = H.replay_rows(H.plane("spikes", rng, 8, 256), -0.01, -0.0, 0)
    assert st["maxpop"].max() >= 16
    _, _, st = H.replay_rows(rng.integers(-3, 4, (8, 64)).astype(np.float32), -0.25, -0.0, 1)
    assert st["scan_tie"].any() and st["read_tie"].any()


def test_dt_quirk_differs_from_true_argmax(oracle):
    rng = np.random.default_rng(7)
    score = rng.standard_normal((23, 31)).astype(np.float32)
    out, Ix, Iy = oracle.dt(score, -0.01, 0.0, -0.01, 0.0, 1, 1)
    ref, ixr, iyr = _dt_brute(score, -0.01, 0.0, -0.01, 0.0, 1, 1)
    true_y = iyr
    assert np.mean(Iy != true_y) > 0.1    # the composition is NOT the true arg-max (Appendix A.3); reproduced on purpose


# ---------------------------------------------------------------------------------- dynamic program
def test_dp_min_against_brute_force_tree(oracle):
    model = M.synthetic_model(seed=5, pa=[0, 1, 1, 2], nmix=2, linear_def=True, anchor_range=2)
    flat = model.flatten()
    rng = np.random.default_rng(3)
    H, W = 7, 9
    resp = rng.standard_normal((flat.nfilters, H, W)).astype(np.float32)
    Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, 0, resp)

    def fid(p, m): return model.filterid[0][p][m]
    children = {p: [c for c in range(model.nparts(0)) if model.parentid[0][c] == p] for p in range(model.nparts(0))}

    def score(p, m):   # full (H, W) accumulated score map of part p, mixture m in float64
        s = resp[fid(p, m)].astype(np.float64).copy()
        for c in children[p]:
            s += message(c, m)
        return s

    def message(c, pm):
        best = np.full((H, W), -np.inf)
        for mm in range(len(model.filterid[0][c])):
            d = model.defid[0][c][mm]
            w = np.float32(model.defw[d]).astype(np.float64)
            ax_, ay_ = model.anchors[d]
            sc = score(c, mm)
            out = np.full((H, W), -np.inf)
            for y in range(H):
                for x in range(W):
                    dx = ax_ + x - np.arange(W)[None, :]
                    dy = ay_ + y - np.arange(H)[:, None]
                    out[y, x] = np.max(sc - w[0] * dx * dx - w[1] * dx - w[2] * dy * dy - w[3] * dy)
            b = np.float32(model.biasw[model.biasid[0][c][mm] + pm])
            best = np.maximum(best, out + float(b))
        return best

    rb = float(np.float32(model.biasw[model.biasid[0][0][0]]))
    ref = np.max(np.stack([score(0, m) + rb for m in range(2)]), axis=0)
    assert np.abs(rootv.astype(np.float64) - ref).max() < 1e-4
    assert np.mean(rooti == np.argmax(np.stack([score(0, m) for m in range(2)]), axis=0)) > 0.98


def test_argmin_boxes_and_order(oracle):
    model = M.synthetic_tiny_model(thresh=0.7)
    flat = model.flatten()
    im = synth.synthetic_frame(5, 96, 128)
    cands = oracle.detect(flat, im)
    assert len(cands) > 0
    keys = [(c["level"], c["component"], c["root_y"], c["root_x"]) for c in cands]
    assert keys == sorted(keys)
    _, scales = oracle.features_pyramid(flat, im)
    for c in cands[:50]:
        assert c["score"] > flat.thresh
        s = np.float32(scales[c["level"]])
        x1 = int(np.rint(np.float32(c["root_x"] - 1) * s)); y1 = int(np.rint(np.float32(c["root_y"] - 1) * s))
        w = int(np.rint(np.float32(5) * s)) - 1
        assert tuple(c["parts"][0]) == (min(x1, x1 + w), min(y1, y1 + w), abs(w), abs(w))   # src/DynamicProgram.cpp:238-244


def test_f64_path_close_to_f32(oracle):
    model = M.synthetic_tiny_model(thresh=0.7)
    flat = model.flatten()
    im = synth.synthetic_frame(5, 96, 128)
    a = oracle.detect(flat, im, dtype=np.float32)
    b = oracle.detect(flat, im, dtype=np.float64)
    ka = {(c["level"], c["root_y"], c["root_x"]): c["score"] for c in a}
    kb = {(c["level"], c["root_y"], c["root_x"]): c["score"] for c in b}
    common = set(ka) & set(kb)
    assert len(common) > 0.95 * max(len(ka), len(kb))
    assert max(abs(ka[k] - kb[k]) for k in common) < 1e-4


# ---------------------------------------------------------------------------------------------------
# image depths other than 8-bit (src/HOGFeatures.cpp:136-146: features<uint16_t|float|double>)
# ---------------------------------------------------------------------------------------------------
def test_hog_of_wider_depths_equals_8bit_on_the_same_values(oracle):
    """The gradient is `*(s+a) - *(s-b)` in the pixel type: for 8-bit-valued pixels stored as uint16 / float / double
    the differences are the same numbers, so features<IT> must give the features<uint8_t> result bit for bit."""
    im8 = synth.synthetic_frame(5, 70, 93, 3)
    for T in (np.float32, np.float64):
        want = oracle.hog_features(im8, 4, 18, 32, T)
        for IT in (np.uint16, np.float32, np.float64):
            got = oracle.hog_features(im8.astype(IT), 4, 18, 32, T)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (T, IT)
    # and a genuinely 16-bit image: scaling every pixel by 256 scales the unnormalised gradients by 256, which the
    # four block normalisations remove up to the 1e-4 epsilon -> same features within 1e-4
    a = oracle.hog_features(im8, 4, 18, 32, np.float64)
    b = oracle.hog_features(im8.astype(np.uint16) * 256, 4, 18, 32, np.float64)
    assert np.abs(a - b).max() < 2e-4


def _np_pyrdown(src, wt, finish):
    r, c, cn = src.shape
    dr, dc = (r + 1) // 2, (c + 1) // 2
    def refl(p, n):
        if n == 1:
            return 0
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p
    s = src.astype(wt)
    rows = np.zeros((r, dc, cn), wt)
    for x in range(dc):
        x0, x1, x2, x3, x4 = refl(2 * x - 2, c), refl(2 * x - 1, c), 2 * x, refl(2 * x + 1, c), refl(2 * x + 2, c)
        rows[:, x] = ((s[:, x2] * wt(6) + (s[:, x1] + s[:, x3]) * wt(4)) + s[:, x0]) + s[:, x4]
    out = np.zeros((dr, dc, cn), wt)
    for y in range(dr):
        y0, y1, y2, y3, y4 = refl(2 * y - 2, r), refl(2 * y - 1, r), refl(2 * y, r), refl(2 * y + 1, r), refl(2 * y + 2, r)
        out[y] = ((rows[y2] * wt(6) + (rows[y1] + rows[y3]) * wt(4)) + rows[y0]) + rows[y4]
    return finish(out)


@pytest.mark.parametrize("IT", [np.uint16, np.float32, np.float64])
def test_pyramid_of_wider_depths_against_numpy(oracle, IT):
    """pyrDown (levels >= interval) against an independent numpy statement of the same taps and operation order;
    level 0 of the pyramid (resize to the same size) is the image itself; 16U-valued-as-8U equals the 8-bit pyramid."""
    rng = np.random.default_rng(3)
    if IT == np.uint16:
        im = rng.integers(0, 65536, (61, 77, 3)).astype(np.uint16)
    else:
        im = (rng.random((61, 77, 3)) * 255).astype(IT)
    imgs, scales = oracle.pyramid_images(im, 4, 3)
    assert imgs[0].dtype == IT and np.array_equal(imgs[0], im)
    for l in range(3, len(imgs)):
        if IT == np.uint16:
            want = _np_pyrdown(imgs[l - 3], np.int64, lambda v: ((v + 128) >> 8).astype(np.uint16))
        elif IT == np.float32:
            want = _np_pyrdown(imgs[l - 3], np.float32, lambda v: v * np.float32(1.0 / 256))
        else:
            want = _np_pyrdown(imgs[l - 3], np.float64, lambda v: v * (1.0 / 256))
        assert imgs[l].shape == want.shape and np.array_equal(imgs[l], want), l
    im8 = synth.synthetic_frame(9, 61, 77, 3)
    a, _ = oracle.pyramid_images(im8, 4, 3)
    b, _ = oracle.pyramid_images(im8.astype(np.uint16), 4, 3)
    for l in range(3, len(a)):              # the integer pyrDown is the same formula; (resized levels use float for 16U)
        if l % 3 == 0:
            assert np.array_equal(a[l], b[l].astype(np.uint8)) and b[l].max() < 256


def test_float_resize_against_numpy(oracle):
    """INTER_LINEAR on float pixels: dst = (S00*a0 + S01*a1)*b0 + (S10*a0 + S11*a1)*b1 with float coefficients
    (1-fx, fx), (1-fy, fy) of the same coordinate mapping as the 8-bit path."""
    rng = np.random.default_rng(4)
    src = (rng.random((37, 53, 1)) * 255).astype(np.float32)
    imgs, _ = oracle.pyramid_images(src, 4, 2)
    dst = imgs[1]
    dr, dc = dst.shape[:2]
    sr, sc = 37, 53
    want = np.zeros((dr, dc), np.float32)
    for dy in range(dr):
        fy = np.float32((dy + 0.5) * (1.0 / (dr / sr)) - 0.5)
        sy = int(np.floor(fy)); fy = np.float32(fy - np.float32(sy))
        y0, y1 = min(max(sy, 0), sr - 1), min(max(sy + 1, 0), sr - 1)
        b0, b1 = np.float32(1) - fy, fy
        for dx in range(dc):
            fx = np.float32((dx + 0.5) * (1.0 / (dc / sc)) - 0.5)
            sx = int(np.floor(fx)); fx = np.float32(fx - np.float32(sx))
            if sx < 0:
                fx, sx = np.float32(0), 0
            if sx >= sc - 1:
                r0, r1 = src[y0, sc - 1, 0], src[y1, sc - 1, 0]
            else:
                a0, a1 = np.float32(1) - fx, fx
                r0 = np.float32(src[y0, sx, 0] * a0) + np.float32(src[y0, sx + 1, 0] * a1)
                r1 = np.float32(src[y1, sx, 0] * a0) + np.float32(src[y1, sx + 1, 0] * a1)
            want[dy, dx] = np.float32(r0 * b0) + np.float32(r1 * b1)
    assert np.array_equal(dst[:, :, 0], want)


# ---------------------------------------------------------------------------------------------------
# the front end on hard frames: the oracle against tests/hog_hard_frames.py's float64 / integer references
# (tests/test_gpu_feature_variants.py ties every kernel variant to the oracle bit for bit on the same frames)
# ---------------------------------------------------------------------------------------------------
HARD_SHAPE = (97, 131)            # odd, no multiple of any sbin used; 24 x 33 blocks at sbin 4, 12 x 16 at sbin 8
GENUINE_SEED = 64                 # the genuine-range frames of this seed hold no pixel next to a bisector (asserted below)
NEAR_TIE = 1e-6                   # relative float64 margin under which a float32 snap may choose the other orientation

# Largest |oracle.hog_features - hog_reference_f64| over every frame of _hog_frames() (8-bit kinds, the same values stored as
# uint16 / float32 / float64, the genuine-range frames), both channel counts, measured on the CPU, and the bar = 4 x measured.
# The deviation is rounding accumulated over the 4 sbin^2 window terms (T = float: also the weights k / sbin, inexact in
# float32 unless sbin is a power of two); 4 x leaves room for other seeds.  No number here comes from a GPU.
#   (sbin, T):        measured     bar
HOG_BARS = {
    (2, "float32"): (8.26e-08, 3.3e-07), (2, "float64"): (1.67e-16, 6.7e-16),
    (3, "float32"): (2.25e-06, 9.0e-06), (3, "float64"): (2.23e-16, 8.9e-16),
    (4, "float32"): (1.03e-07, 4.1e-07), (4, "float64"): (2.23e-16, 8.9e-16),
    (5, "float32"): (1.92e-06, 7.7e-06), (5, "float64"): (3.34e-16, 1.3e-15),
    (6, "float32"): (1.02e-06, 4.1e-06), (6, "float64"): (2.78e-16, 1.1e-15),
    (8, "float32"): (1.02e-07, 4.1e-07), (8, "float64"): (2.78e-16, 1.1e-15),
}
# Typed resize (16U / 32F / 64F): largest |oracle level - resize_linear_reference| over the resized levels, relative to the
# frame's largest |pixel| (16U: in units, after the round; one unit is the bar), and 4 x that.  The float pyrDown, against
# the float64 sum / 256, likewise (the taps are exact, the 24 additions round).  Every integer pyrDown is exact: no bar.
#   dtype:            resize measured, bar      pyrDown measured, bar
RESAMPLE_BARS = {
    "uint16": (1, 1, 0, 0),
    "float32": (1.15e-07, 4.6e-07, 1.53e-07, 6.1e-07),
    "float64": (0.0, 0.0, 5.55e-16, 2.2e-15),          # the double resize is the reference's own sequence of operations: equal
}

_hog_ref_cache = {}


def _hog_ref(key, im, sbin):
    if (key, sbin) not in _hog_ref_cache:
        _hog_ref_cache[key, sbin] = F.hog_reference_f64(im, sbin)
    return _hog_ref_cache[key, sbin]


def _hog_frames(cn):
    """name -> (frame, genuine): the 8-bit kinds (near_bisector also as three 200 x 200 frames: the 3072 pairs with the smallest
    margin), the scene and noise stored as the wider types, and the genuine-range frames"""
    out = {name: (im, False) for name, im in F.frames_u8(40, *HARD_SHAPE, cn).items()}
    for part in range(3):
        out[f"near_bisector_200_{part}"] = (F.near_bisector(200, 200, cn, part), False)
    for IT in (np.uint16, np.float32, np.float64):
        for name in ("scene", "noise", "vertical"):
            out[f"{name}_as_{IT.__name__}"] = (out[name][0].astype(IT), False)
        for name, im in F.frames_genuine(IT, GENUINE_SEED, *HARD_SHAPE, cn).items():
            out[f"{name}_{IT.__name__}"] = (im, True)
    return out


def hog_deviation(oracle, sbin, T, cn):
    """largest deviation of the compared cells over _hog_frames(cn), per frame: {name: (deviation, cells left out, cells)}"""
    res = {}
    for name, (im, genuine) in _hog_frames(cn).items():
        if name == "texture_float64" and T == np.float32:
            continue        # by construction every gradient of it is within 2^-22 of an 8-bit one: all near-ties in float32
        ref, margin = _hog_ref((name, cn), im, sbin)
        got = oracle.hog_features(im, sbin, dtype=T)
        assert got.dtype == T and got.shape == ref.shape, (name, got.shape, ref.shape)
        d = np.abs(got.astype(np.float64) - ref).reshape(ref.shape[0], -1, 32).max(axis=2)
        # integer gradients (every frame that is not `genuine`) need no exclusion, nor does T = double against float64
        skip = F.cells_fed_by(margin, NEAR_TIE) if genuine and T == np.float32 else np.zeros(d.shape, bool)
        res[name] = (float(d[~skip].max()) if (~skip).any() else 0.0, int(skip.sum()), int(skip.size))
    return res


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("sbin", F.SBINS)
def test_hog_on_hard_frames_against_float64_reference(oracle, sbin, T, cn):
    """oracle.hog_features at every bin size pbd_create accepts a model for, both real types, grey and colour, on the hard
    frames: every cell within HOG_BARS of the float64 scatter form.  On integer gradients the float32 and the float64 snap
    choose the same orientation (test_integer_gradients_snap_alike), so every cell is compared; on the genuine-range frames
    a cell is left out for T = float only when a pixel feeding it lies within 1e-6 (relative) of a bisector, and at most
    0.5 % of a frame's cells are."""
    measured, bar = HOG_BARS[sbin, np.dtype(T).name]
    assert bar <= 4.05 * measured
    for name, (dev, left_out, cells) in hog_deviation(oracle, sbin, T, cn).items():
        assert left_out <= 0.005 * cells, (name, left_out, cells)
        assert dev <= bar, (name, dev, bar)


def test_integer_gradients_snap_alike():
    """All 261 121 8-bit gradient pairs: the float32 scan and the float64 scan choose the same orientation, and the only exact
    ties are the 511 pairs with dx == 0 (dots 4 and 5; (0, 0) ties everything), which the strict `>` resolves to 4 / 13."""
    dy, dx = np.mgrid[-255:256, -255:256]
    dx, dy = dx.ravel(), dy.ravel()

    def scan(R):
        best, ori = np.zeros(dx.size, R), np.zeros(dx.size, np.int64)
        for k in range(9):
            dot = R(F.UU[k]) * dx.astype(R) + R(F.VV[k]) * dy.astype(R)
            up, down = dot > best, ~(dot > best) & (-dot > best)
            best = np.where(up, dot, np.where(down, -dot, best))
            ori = np.where(up, k, np.where(down, k + 9, ori))
        return ori

    o32, o64 = scan(np.float32), scan(np.float64)
    assert np.array_equal(o32, o64)
    ori, best, gap = F.snap_f64(dx.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(ori, o64)
    assert np.array_equal(gap == 0, dx == 0) and np.count_nonzero(gap == 0) == 511
    assert set(o64[(dx == 0) & (dy > 0)]) == {4} and set(o64[(dx == 0) & (dy < 0)]) == {13}


def test_hard_frames_hold_what_they_are_for():
    """the frames' own claims, so that a change to a builder cannot quietly empty a case"""
    rows, cols = HARD_SHAPE
    ext = F.extremes(rows, cols, 3)
    assert set(np.unique(ext)) == {0, 255}
    d = ext[1:-1, 2:].astype(int) - ext[1:-1, :-2]
    assert (d == 255).any() and (d == -255).any() and (d == 0).any()
    ver = F.vertical(3, rows, cols, 1)[:, :, 0].astype(int)
    dx, dy = ver[1:-1, 2:] - ver[1:-1, :-2], ver[2:, 1:-1] - ver[:-2, 1:-1]
    assert np.mean((dx == 0) & (dy != 0)) > 0.5 and ((dx == 0) & (dy > 0)).any() and ((dx == 0) & (dy < 0)).any()
    tie = F.channel_ties(rows, cols).astype(int)
    dx, dy = tie[1:-1, 2:] - tie[1:-1, :-2], tie[2:, 1:-1] - tie[:-2, 1:-1]
    v = dx * dx + dy * dy
    all3 = (v[:, :, 0] == v[:, :, 1]) & (v[:, :, 1] == v[:, :, 2]) & (v[:, :, 0] > 0)
    assert all3.sum() >= 40 and len({(int(a), int(b)) for a, b in zip(dx[all3][:, 2], dy[all3][:, 2])}) >= 6
    for hi, lo in ((2, 1), (2, 0), (1, 0), (1, 2), (0, 2), (0, 1)):          # two channels tie above the third, each way
        other = 3 - hi - lo
        assert ((v[:, :, hi] == v[:, :, other]) & (v[:, :, lo] < v[:, :, hi]) & (v[:, :, lo] > 0)).any() or \
               ((v[:, :, hi] == v[:, :, lo]) & (v[:, :, other] < v[:, :, hi]) & (v[:, :, other] > 0)).any()
    pairs = F.near_bisector_pairs()
    assert (pairs[:510, 0] == 0).all() and (pairs[510:3072, 0] != 0).all()
    nb = F.near_bisector(200, 200, 1, 1)[:, :, 0].astype(int)                # part 1: past the exact ties
    dx, dy = nb[1:-1, 2:] - nb[1:-1, :-2], nb[2:, 1:-1] - nb[:-2, 1:-1]
    _, best, gap = F.snap_f64(dx.astype(float), dy.astype(float))
    centre = (dx != 0) & (dy != 0)
    assert centre.sum() >= 1000 and np.sort(gap[centre] / best[centre])[999] < 1e-3
    for IT in (np.float32, np.float64):
        g = F.frames_genuine(IT, GENUINE_SEED, rows, cols, 3)
        assert 0 <= g["unit"].min() and g["unit"].max() <= 1.001 and g["wide"].min() < -900 and g["wide"].max() > 900
    g16 = F.frames_genuine(np.uint16, GENUINE_SEED, rows, cols, 3)["full"]
    assert g16.min() == 0 and g16.max() == 65535


def resample_deviation(oracle, im, exact_first=False):
    """(resize deviation, pyrDown deviation) of oracle.pyramid_images(im, 4, 3) against the references, level by level; exact
    comparisons are asserted here (exact_first: level 3, the pyrDown of the frame itself, of an 8-bit-valued float frame)"""
    imgs, _ = oracle.pyramid_images(im, 4, 3)
    assert len(imgs) > 3 and imgs[0].dtype == im.dtype
    scale = 1.0 if im.dtype.kind == "u" else float(np.abs(im).max())
    dev_r = dev_p = 0.0
    for l, got in enumerate(imgs):
        if l < 3:
            if im.dtype == np.uint8:
                assert np.array_equal(got, F.resize_u8_reference(im, *got.shape[:2])), l
            elif l == 0:
                assert np.array_equal(got, im)                           # the same size: the image itself
            else:
                ref = F.resize_linear_reference(im, *got.shape[:2])
                dev_r = max(dev_r, float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) / scale)
        else:
            ref = F.pyrdown_reference(imgs[l - 3])
            if im.dtype.kind == "u" or (exact_first and l == 3):
                assert np.array_equal(got, ref), l
            else:
                dev_p = max(dev_p, float(np.abs(got.astype(np.float64) - ref).max()) / scale)
    return dev_r, dev_p


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("IT", [np.uint8, np.uint16, np.float32, np.float64])
def test_pyramid_images_of_every_depth_against_the_references(oracle, IT, cn):
    """oracle.pyramid_images, interval 3, one shape.  8U: resized levels and pyrDown levels integer-exact.  16U: pyrDown
    integer-exact, resize within one unit of the float64 bilinear value rounded half to even.  32F / 64F: the pyrDown of an
    8-bit-valued frame itself exactly (every sum and the final * 1/256 are exact); the pyrDown of resized levels and of
    genuine-range frames, and the resize, within RESAMPLE_BARS."""
    frames = F.frames_u8(40, *HARD_SHAPE, cn)
    if IT == np.uint8:
        for name, im in frames.items():
            resample_deviation(oracle, im)
        return
    r_meas, r_bar, p_meas, p_bar = RESAMPLE_BARS[np.dtype(IT).name]
    assert r_bar <= 4.05 * r_meas and p_bar <= 4.05 * p_meas
    for name in ("scene", "noise", "extremes"):
        dev_r, dev_p = resample_deviation(oracle, frames[name].astype(IT), exact_first=True)
        assert dev_r <= r_bar and dev_p <= p_bar, (name, dev_r, dev_p)
    for name, im in F.frames_genuine(IT, GENUINE_SEED, *HARD_SHAPE, cn).items():
        dev_r, dev_p = resample_deviation(oracle, im)
        assert dev_r <= r_bar and dev_p <= p_bar, (name, dev_r, dev_p)
