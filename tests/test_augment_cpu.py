"""The augmentation rule on the CPU (partsbaseddetector_amd/augment.py): the yardstick's invariants, an
independent per-pixel formulation, the point maps, the mirror check, the order of the extended list, the host functions of the
library (pbd_augment_plan, pbd_augment_points: the library loads without a GPU) and the training case the GPU test compares on.
No GPU is needed."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd import augment as A

import augment_cases as AC

SMALL = AC.SHAPES[:5]


def image(shape, cn=3, seed=0):
    return np.random.default_rng(seed).integers(1, 256, tuple(shape) + (cn,)).astype(np.uint8)


# ---- the yardstick's invariants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AC.SHAPES)
def test_zero_degrees_is_the_identity_and_mirror_twice_too(shape):
    im = image(shape)
    assert np.array_equal(A.rotate_ref(im, 0.0), im)
    assert np.array_equal(A.rotate_ref(im, -0.0), im)
    m = A.rotate_ref(im, 0.0, mirror=True)
    assert np.array_equal(m, im[:, ::-1]) and np.array_equal(A.rotate_ref(m, 0.0, mirror=True), im)
    assert np.array_equal(A.rotate_ref(im[:, :, 0], 0.0, mirror=True), im[:, ::-1, 0])


@pytest.mark.parametrize("shape", AC.SHAPES)
def test_quarter_turn_is_rot90_inside_the_padding(shape):
    """odd and even sizes: the block np.rot90(im, 1) stands somewhere in the output and everything around it is zero"""
    im = image(shape)
    out = A.rotate_ref(im, 90.0)
    want = np.rot90(im, 1)
    hits = [(i, j) for i in range(out.shape[0] - want.shape[0] + 1) for j in range(out.shape[1] - want.shape[1] + 1)
            if np.array_equal(out[i:i + want.shape[0], j:j + want.shape[1]], want)]
    assert len(hits) == 1
    assert np.count_nonzero(out.any(axis=2)) == want.shape[0] * want.shape[1]      # no pixel of im is zero
    assert np.array_equal(A.rotate_ref(im, 90.0 - 360.0), out) and np.array_equal(A.rotate_ref(im, 450.0), out)


def formula_size(rows, cols, c, s):
    """section 1's formula, written apart from augment._geometry"""
    hr, hc = (rows - 1) / 2, (cols - 1) / 2
    corners = [(-hr * c - hc * s, -hr * s + hc * c), (hr * c - hc * s, hr * s + hc * c)]
    return tuple(int(2 * (math.ceil(max(abs(p[k]) for p in corners) / 2) * 2) + 1) for k in (0, 1))


@pytest.mark.parametrize("shape", AC.SHAPES)
def test_output_sizes_follow_the_formula(shape):
    for d in AC.DEGREES + (360.0, -90.0, 123.456):
        orows, ocols, (c, s) = A.plan(shape[0], shape[1], d)
        if d == 0:
            assert (orows, ocols) == shape
            continue
        assert (orows, ocols) == formula_size(shape[0], shape[1], c, s)
        assert orows % 4 == 1 and ocols % 4 == 1
        assert A.rotate_ref(image(shape, 1), d).shape[:2] == (orows, ocols)
    assert A.coefficients(90.0) == (0.0, 1.0) and A.coefficients(180.0) == (-1.0, 0.0) and A.coefficients(-90.0) == (0.0, -1.0)
    assert A.coefficients(360.0) == (1.0, 0.0) and A.plan(5, 4, 360.0)[:2] == (5, 5)     # a rotation step, unlike 0


def loop_rotate(im, degrees, mirror):
    """the rule pixel by pixel in Python floats: an independent formulation of rotate_ref"""
    rows, cols = im.shape[:2]
    orows, ocols, (c, s) = A.plan(rows, cols, degrees)
    out = np.zeros((orows, ocols) + im.shape[2:], im.dtype)
    hAr, hAc, hBr, hBc = (rows - 1) / 2, (cols - 1) / 2, (orows - 1) // 2, (ocols - 1) // 2
    for R in range(orows):
        for Q in range(ocols):
            if degrees == 0:
                r, q = R, Q
            else:
                r = math.floor((R - hBr) * c + (Q - hBc) * s + hAr + 0.5)
                q = math.floor(-((R - hBr) * s) + (Q - hBc) * c + hAc + 0.5)
            if 0 <= r < rows and 0 <= q < cols:
                out[R, Q] = im[r, cols - 1 - q] if mirror else im[r, q]
    return out


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("shape", SMALL)
def test_per_pixel_loop_equals_the_vectorised_yardstick(shape, mirror):
    for cn, dtype in ((3, np.uint8), (1, np.float64)):
        im = AC.frames(dtype, cn)[AC.SHAPES.index(shape)]
        for d in AC.DEGREES:
            assert loop_rotate(im, d, mirror).tobytes() == A.rotate_ref(im, d, mirror).tobytes(), (d, cn)


# ---- points -----------------------------------------------------------------------------------------------------------------
def inverse_points(xy, rows, cols, degrees, mirror):
    """map_rotate_points.m:42 (new2ori), then the mirror undone"""
    orows, ocols, (c, s) = A.plan(rows, cols, degrees)
    x, y = xy[:, 0], xy[:, 1]
    if degrees != 0:
        u, v = y - (orows - 1) / 2, x - (ocols - 1) / 2
        y, x = (u * c + v * s) + (rows - 1) / 2, (-(u * s) + v * c) + (cols - 1) / 2
    if mirror:
        x = (cols - 1) - x
    return np.stack([x, y], axis=1)


def test_points_round_trip_through_the_inverse_map():
    rng = np.random.default_rng(2)
    for shape in AC.SHAPES:
        pts = rng.uniform(-3, max(shape) + 3, (20, 2))
        for d in AC.DEGREES:
            for m in (False, True):
                fwd = A.points_ref(pts, shape[0], shape[1], d, m)
                back = inverse_points(fwd, shape[0], shape[1], d, m)
                assert np.abs(back - pts).max() < 1e-9, (shape, d, m)
    assert np.array_equal(A.points_ref([[2.0, 1.0]], 5, 4, 0.0, True), [[1.0, 1.0]])


def test_a_block_around_a_point_is_found_at_the_mapped_point():
    """a 3 x 3 block of one value around an integer point: the output pixel at the rounded mapped point holds that value, mirrored
    or not, no case excepted (the rounded point is at most 0.5 * sqrt(2) from the mapped one, the block reaches 1.5 around it)"""
    rng = np.random.default_rng(3)
    n = 0
    for shape in ((17, 9), (48, 64), (31, 40)):
        for d in AC.DEGREES[1:] + (123.0, -61.7):
            for _ in range(25):
                for m in (False, True):
                    y, x = int(rng.integers(1, shape[0] - 1)), int(rng.integers(1, shape[1] - 1))
                    im = np.zeros(shape, np.uint8)
                    im[y - 1:y + 2, x - 1:x + 2] = 200
                    out = A.rotate_ref(im, d, m)
                    px, py = A.points_ref([[x, y]], shape[0], shape[1], d, m)[0]
                    assert out[int(math.floor(py + 0.5)), int(math.floor(px + 0.5))] == 200, (shape, d, m, x, y)
                    n += 1
    assert n >= 1400


# ---- the library's host functions -------------------------------------------------------------------------------------------
def test_library_plan_and_points_equal_the_yardstick():
    rng = np.random.default_rng(4)
    for shape in AC.SHAPES + ((480, 640), (32000, 1)):
        for d in AC.DEGREES + (360.0, -450.0, 1e6, 123.456):
            orows, ocols, coef = A.plan_c(shape[0], shape[1], d)
            assert (orows, ocols) == A.plan(shape[0], shape[1], d, coef if d else None)[:2]
            if math.fmod(d, 90.0) == 0:
                assert coef == A.coefficients(d)
            pts = rng.uniform(-5, 700, (9, 2))
            for m in (False, True):
                want = A.points_ref(pts, shape[0], shape[1], d, m, coef if d else None)
                assert A.points_c(pts, shape[0], shape[1], d, m).tobytes() == want.tobytes(), (shape, d, m)
    assert A.points_c(np.zeros((0, 2)), 5, 4, 15.0).shape == (0, 2)


@pytest.mark.parametrize("args", [(0, 4, 15.0), (5, 0, 15.0), (32001, 4, 15.0), (5, 4, float("nan")), (5, 4, float("inf"))])
def test_library_refuses_bad_plans(args):
    from partsbaseddetector_amd._lib import PbdError
    with pytest.raises(PbdError) as e:
        A.plan_c(*args)
    assert e.value.code == -1
    with pytest.raises(PbdError):
        A.points_c([[1.0, 1.0]], *args)
    with pytest.raises(ValueError):
        A.plan(*args)


# ---- the mirror permutation and the extended list ---------------------------------------------------------------------------
def test_check_mirror():
    pa = [0, 1, 2, 3, 2, 5]                 # a trunk 0 - 1 with two arms 2 - 3 and 4 - 5
    assert A.check_mirror([0, 1, 4, 5, 2, 3], pa).tolist() == [0, 1, 4, 5, 2, 3]
    assert A.check_mirror(range(6), pa).tolist() == list(range(6))
    with pytest.raises(ValueError, match="involution"):
        A.check_mirror([0, 1, 3, 4, 2, 5], pa)           # a 3-cycle
    with pytest.raises(ValueError, match="tree"):
        A.check_mirror([0, 1, 5, 3, 4, 2], pa)           # an involution that swaps an arm's end with the other arm's start
    with pytest.raises(ValueError, match="permutation"):
        A.check_mirror([0, 1, 2, 2, 4, 5], pa)
    with pytest.raises(ValueError, match="permutation"):
        A.check_mirror([0, 1, 2], pa)


def test_augment_positives_ref_order_and_count():
    pos = [{"im": image((17, 9), seed=n), "points": np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]) + n} for n in range(3)]
    perm = [0, 2, 1]
    out = A.augment_positives_ref(pos, (15.0, -30.0), perm)
    assert len(out) == 3 * 6 and A.copies((15.0, -30.0), perm) == [(False, 0.0), (False, 15.0), (False, -30.0), (True, 0.0),
                                                                    (True, 15.0), (True, -30.0)]
    for n, p in enumerate(pos):
        for k, (m, d) in enumerate(A.copies((15.0, -30.0), perm)):
            got = out[6 * n + k]
            assert sorted(got) == ["im", "points"]
            assert got["im"].tobytes() == A.rotate_ref(p["im"], d, m).tobytes()
            src = p["points"][perm] if m else p["points"]
            assert got["points"].tobytes() == A.points_ref(src, 17, 9, d, m).tobytes()
        assert np.array_equal(out[6 * n]["im"], p["im"]) and np.array_equal(out[6 * n]["points"], p["points"])
        assert np.array_equal(out[6 * n + 3]["points"][1], [8 - p["points"][2][0], p["points"][2][1]])   # part 1 <- mirrored part 2
    assert len(A.augment_positives_ref(pos, (15.0,), None)) == 6 and len(A.augment_positives_ref(pos, (), None)) == 3
    with pytest.raises(ValueError):
        A.augment_positives_ref(pos, (float("nan"),), None)


# ---- the training case of tests/test_gpu_train_augment.py -------------------------------------------------------------------
def test_training_case_is_not_empty():
    """trainmodel_ref completes on the augmented case, every (part, type) has a positive, and rotated and mirrored copies are
    among the latent positives: the GPU comparison cannot pass on an empty set"""
    from partsbaseddetector_amd import trainmodel as TM
    pos, neg, kw, aug = AC.train_case()
    assert len(pos) <= 4 and len(aug["degrees"]) == 1 and aug["mirror"] is not None
    model, info = AC.ref_run()
    assert info["augment"] == {"degrees": [15.0], "mirror": [0, 1, 2], "copies": AC.COPIES, "total": AC.COPIES * len(pos)}
    assert info["idx"].shape == (3, AC.COPIES * len(pos))
    for p, k in enumerate(kw["K"]):
        for t in range(k):
            assert np.any(info["idx"][p] == t)
            assert info["part_info"][p][t]["numpositives"][0] >= 1
    for name in ("final1", "final"):
        f = info[name]
        latent = set(range(AC.COPIES * len(pos))) - set(f["skipped"]) - set(f["notfound"])
        assert sum(f["numpositives"]) == len(latent) >= 8
        assert any(n % AC.COPIES == 1 for n in latent), "no rotated copy among the latent positives"
        assert any(n % AC.COPIES == 2 for n in latent), "no mirrored copy among the latent positives"
        assert any(n % AC.COPIES == 3 for n in latent)
    with pytest.raises(ValueError):
        TM.trainmodel_ref(pos, neg, dtype=np.float32, augment={"degrees": (15.0,), "mirror": [1, 0, 2]}, **kw)
    with pytest.raises(ValueError):
        TM.trainmodel_ref(pos, neg, dtype=np.float32, augment={"angle": (15.0,)}, **kw)
