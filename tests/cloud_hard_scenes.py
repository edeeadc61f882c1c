"""Built hard inputs for plane removal and object clustering (tests/test_cloud_hard_cpu.py, tests/test_gpu_cloud_hard.py).

Builders only: numpy, no handle, no randomness beyond fixed seeds, so every machine builds the same inputs.  A plane scene is a
dict of PlaneCall (the clouds of one call, its PlaneParams); a cluster scene is a dict of ClusterCall (clouds, boxes, frames).
What each scene is built to reach is asserted from the yardstick alone in tests/test_cloud_hard_cpu.py; DESIGN.md section 6e, "Built hard clouds"
has the table of scenes, kernels and branches.

The sizes named here restate constants of the kernels (csrc/pbd_internal.h, pbd_kernels_planes.hip, pbd_kernels_cloud.hip,
pbd_device.h): a scene that crosses one of them says which.
"""
from collections import namedtuple

import numpy as np

from partsbaseddetector_amd.pointcloud import PinholeCamera, PlaneParams, PointCloudClusterer, cloud_from_depth

REF_LDS_ROWS = 4096      # kPlRefLds: taller clouds exchange the refinement wavefront through global memory
REF_THREADS = 1024       # kRefThreads: rows per thread stride of k_pl_refine
MAX_GRID = 4096          # kPlMaxGrid / kClMaxGrid: more work items than this make a kernel grid-stride
MOMENT_ROWS = 128        # kMoRows: rows per round of k_pl_moments
SCAN_TILE = 1024         # kScanTile = kClChunk: points per scan tile and per crop chunk
SELECT_ROUND = 256       # boxes per round of k_cl_select, points per round of k_cl_out
HOST_CROP = 65536        # the host form's first crop capacity

F = np.float32
NAN = np.nan

PlaneCall = namedtuple("PlaneCall", "clouds params")
ClusterCall = namedtuple("ClusterCall", "clouds boxes frames")


# ---- plane scenes -------------------------------------------------------------------------------------------------------------
def sheet(rows, cols, z0=2.0, ax=0.0, ay=0.0, step=0.005, x0=0.0, y0=0.0):
    """an organized cloud seen straight on: x = x0 + c * step, y = y0 + r * step, z = z0 + ax * x + ay * y, rounded to float32"""
    r, c = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x0 + c * step, y0 + r * step
    return np.stack([x, y, z0 + ax * x + ay * y], axis=-1).astype(np.float32)


def checker(rows, cols):
    """every pixel a depth edge (z alternates between 1 and 1.5): no normal anywhere, so no two points join"""
    P = sheet(rows, cols)
    r, c = np.mgrid[0:rows, 0:cols]
    P[..., 2] = np.where((r + c) % 2 == 0, 1.0, 1.5)
    return P


def tall_plane(rows, cols):
    """a tilted plane with a small NaN hole; 2 mm rows keep z between 2 and 2.5 m over 4100 rows"""
    P = sheet(rows, cols, 2.0, 0.1, 0.05, step=0.002)
    P[rows // 3:rows // 3 + 3, cols // 2:cols // 2 + 2] = NAN
    return P


def tall():
    q = PlaneParams(min_inliers=100)
    a, b = tall_plane(REF_LDS_ROWS + 1, 13), tall_plane(REF_LDS_ROWS + 4, 24)
    return {
        "4097x13": PlaneCall([a], q),
        "4100x24": PlaneCall([b], q),
        "small_4100_4097": PlaneCall([tall_plane(40, 30), b, a], q),         # both tall slices of xch at rbase != 0
        "1024x16_1025x16": PlaneCall([tall_plane(REF_THREADS, 16), tall_plane(REF_THREADS + 1, 16)], q),
    }


def corridor_mask(rows, cols, pitch=14, wall=2, gap=12, mode="snake"):
    """True where a NaN wall stands.  Vertical walls every `pitch` columns; "snake": they leave a gap alternately at the bottom
    and at the top (one serpentine corridor); "comb": all leave the gap at the bottom (teeth joined by the bottom strip)"""
    m = np.zeros((rows, cols), bool)
    for k, c in enumerate(range(pitch - wall, cols - wall, pitch)):
        if mode == "snake" and k % 2:
            m[gap:, c:c + wall] = True
        else:
            m[:rows - gap, c:c + wall] = True
    return m


def snake():
    q = PlaneParams(smoothing_size=4)
    P = sheet(240, 320)
    s = P.copy()
    s[corridor_mask(240, 320)] = NAN
    c = P.copy()
    m = corridor_mask(240, 320, mode="comb")
    m[:, 158:162] = True                                    # two combs ...
    m[240 - 12:, 158:162] = False                           # ... whose bottom strips meet
    m[120:240 - 12, 40:300:28] = True                       # and teeth split once more half way down
    c[m] = NAN
    return {
        "snake": PlaneCall([s], q),
        "snake_T": PlaneCall([np.ascontiguousarray(s.transpose(1, 0, 2))], q),
        "comb": PlaneCall([c], q),
    }


def patch_field(n, size=7, gap=1, zstep=0.001):
    """n x n flat square patches on NaN, each at its own depth: with smoothing_size 2 a 7 x 7 patch has a 3 x 3 core of points
    with normals (one segment of 9) and two rings that only refinement can label"""
    pitch = size + gap
    P = sheet(n * pitch, n * pitch)
    z = np.full(P.shape[:2], NAN)
    for i in range(n):
        for j in range(n):
            z[i * pitch:i * pitch + size, j * pitch:j * pitch + size] = 2.0 + zstep * (i * n + j)
    P[..., 2] = z
    P[np.isnan(z)] = NAN
    return P


def singles():
    return {
        "checker_70x70": PlaneCall([checker(70, 70)], PlaneParams(min_inliers=0)),       # 4900 candidates > kPlMaxGrid
        "patches_15x15": PlaneCall([patch_field(15)], PlaneParams(smoothing_size=2, min_inliers=4)),   # 225 planes
    }


def far():
    """a tilted plane about 400 m off the axis (cx = -60000): the double moments are large enough for their order to show in the
    float32 coefficients.  200 rows > kMoRows and 300 columns > 64: rounds, ballot tiles and waves all take part."""
    rows, cols = 200, 300
    cam = PinholeCamera(525.0, 525.0, -60000.0, 99.5)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rx, ry = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
    d = 400.0 / (rx + 0.25 * ry + 1.0)                    # the plane x + 0.25 y + z = 400
    return {"far": PlaneCall([cloud_from_depth(d.astype(np.float32), cam)], PlaneParams())}


def special_values():
    """a flat 24 x 24 cloud with +Inf, -Inf, zero and negative z, and coordinates near 1e30 whose products overflow"""
    P = sheet(24, 24)
    P[3, 3, 0] = np.inf
    P[3, 9, 2] = -np.inf
    P[9, 3, 2] = 0.0
    P[9, 9, 2] = -2.0
    P[15, 15] = (1e30, -1e30, 1e30)
    P[20, 5] = (3e38, 3e38, 3e38)
    P[23, 23] = (0.0, 0.0, -0.0)
    return P


def edges():
    flat = lambda r, c: sheet(r, c, 2.0, 0.05, 0.02)
    s1 = PlaneParams(smoothing_size=2, min_inliers=0)
    out = {
        # default smoothing (s = 5): 12 = 2s+2 has no valid centre, 13 = 2s+3 exactly one
        "around_2s+3": PlaneCall([flat(12, 40), flat(13, 40), flat(40, 12), flat(40, 13), flat(13, 13), flat(12, 12)],
                                 PlaneParams(min_inliers=20)),
        # s = 1: one row of 1, 2, 3 and 5 valid centres: single points and collinear segments as candidates
        "collinear": PlaneCall([flat(5, 5), flat(5, 6), flat(5, 7), flat(5, 9), flat(6, 5), flat(7, 5), flat(4, 9), flat(9, 4)], s1),
        "ballot_tiles": PlaneCall([flat(140, 64), flat(140, 65), flat(140, 63)], PlaneParams(min_inliers=500)),
        "moment_rounds": PlaneCall([flat(MOMENT_ROWS, 70), flat(MOMENT_ROWS + 1, 70), flat(2 * MOMENT_ROWS + 1, 20)],
                                   PlaneParams(min_inliers=500)),
        "special_values": PlaneCall([special_values()], PlaneParams(smoothing_size=2, min_inliers=4)),
    }
    # point counts around the scan tile, alone in their call so the count is the call's: flat (planes) and checker (every point
    # a kept one-point candidate, the last one included)
    for rows, cols in ((31, 33), (32, 32), (25, 41), (3, 683), (64, 32), (683, 3)):
        n = rows * cols
        out["flat_%d" % n if rows != 683 else "flat_%dT" % n] = PlaneCall([flat(rows, cols)], PlaneParams(smoothing_size=2, min_inliers=4))
        out["checker_%d" % n if rows != 683 else "checker_%dT" % n] = PlaneCall([checker(rows, cols)], s1)
    return out


STAIRS = [(12, 11), (12, 10)] + [(12 - k, c - k) for k in range(1, 6) for c in (12, 11, 10)]


def refine():
    """Label situations of the refinement recurrence, one guard each.  Every patch is flat at z = 2 (its fitted plane is
    exactly (0, 0, -1, 2)); the points under test hang off a patch and have NaN elsewhere around them, so exactly one rule
    decides each.  distance_threshold = 1/32: at z = 2 the absorb threshold is 0.125 exactly."""
    q = PlaneParams(smoothing_size=2, min_inliers=4, distance_threshold=0.03125)

    def blank(rows, cols):
        P = sheet(rows, cols)
        z = np.full((rows, cols), NAN)
        return P, z

    def done(P, z):
        P = P.copy()
        P[..., 2] = z
        P[np.isnan(z)] = NAN
        return P

    out = {}
    # upper neighbour a plane, (r-1, c+1) not finite: X below the patch's lower right corner stays unlabelled
    P, z = blank(14, 14)
    z[1:10, 1:10] = 2.0
    z[10, 9] = 2.0
    out["upper_right_nan"] = PlaneCall([done(P, z)], q)
    # the same with (r-1, c+1) finite: X is absorbed from above
    P, z = blank(14, 14)
    z[1:10, 1:10] = 2.0
    z[10, 8] = 2.0
    out["upper_right_finite"] = PlaneCall([done(P, z)], q)
    # last column: the patch touches the right border, X hangs below it in the last column
    P, z = blank(14, 12)
    z[1:10, 3:12] = 2.0
    z[10, 11] = 2.0
    out["last_column"] = PlaneCall([done(P, z)], q)
    # last row: the patch touches the bottom border; (H-2, c) beside it is finite but far (3 m), X = (H-1, c) is at 2 m
    P, z = blank(12, 14)
    z[3:12, 1:10] = 2.0
    z[10, 10] = 3.0
    z[11, 10] = 2.0
    out["last_row"] = PlaneCall([done(P, z)], q)
    # two planes: A (2 m) above, B (2.0625 m) to the left with an arm along row 11; X = (11, 16) lies under a point of A and right
    # of the arm's end, within both thresholds: the upper plane wins.  Both neighbours are labelled in the forward pass (each is
    # reached from its core by steps right and down), and row 10 is NaN over the arm, so A does not take the arm from above.
    P, z = blank(24, 24)
    z[1:10, 12:21] = 2.0
    z[10, 16:18] = 2.0
    z[6:15, 2:11] = 2.0625
    z[11, 11:16] = 2.0625
    z[11, 16] = 2.03125
    out["upper_beats_left"] = PlaneCall([done(P, z)], q)
    # a staircase up and to the left of the patch (STAIRS): the forward pass, which hands labels right and down, never reaches
    # it; the backward pass fills it, each step from the right or from below (where the point diagonally below is finite)
    P, z = blank(24, 24)
    z[12:21, 12:21] = 2.0
    for p in STAIRS:
        z[p] = 2.0
    out["staircase"] = PlaneCall([done(P, z)], q)
    # thresholds: X right of the patch.  |2 - z(X)| against 0.03125 * z^2 with z of the patch point (2 -> 0.125) or of X
    P, z = blank(14, 16)
    z[1:10, 1:10] = 2.0
    z[2, 10] = 2.125          # distance 0.125 = the threshold at z = 2 exactly: not absorbed (<), absorbed by <= or by z of X
    z[4, 10] = 1.875          # distance 0.125 again, from the near side: z of X gives 0.1099, still not absorbed
    z[6, 10] = np.nextafter(F(2.125), F(0))      # one ulp inside: absorbed
    z[8, 10] = 1.8828125      # distance 0.1171875: absorbed with z = 2 (0.125), not with z of X (0.11078)
    out["thresholds"] = PlaneCall([done(P, z)], q)
    return out


def many():
    """one call of about 40 clouds of mixed shapes, each compared with its single-cloud yardstick"""
    q = PlaneParams(smoothing_size=4, min_inliers=60)
    clouds = [sheet(2, 2), sheet(2, 37), sheet(37, 2), np.full((9, 11, 3), NAN, np.float32)]
    for k in range(14):
        clouds.append(sheet(11 + 3 * k, 40 - 2 * k, 2.0 + 0.1 * k, 0.02 * k, -0.03 * k))
    clouds.append(tall_plane(REF_LDS_ROWS + 1, 13))
    clouds.append(np.full((2, 2, 3), NAN, np.float32))
    s = sheet(90, 100)
    s[corridor_mask(90, 100)] = NAN
    clouds.append(s)
    clouds.append(patch_field(4, size=9))
    for k in range(14):
        c = checker(3 + k, 5 + 2 * k) if k % 3 == 0 else sheet(20 + k, 21 + 5 * k, 1.5, 0.3, 0.1)
        clouds.append(c)
    clouds += [special_values(), sheet(2, 2), tall_plane(REF_THREADS + 1, 9)]
    return {"many": PlaneCall(clouds, q)}


def bowl(tilt_x=0.0, tilt_y=0.0, n=60):
    """a curved surface: neighbouring normals and plane distances differ a little more at every pixel, so both join tests change
    sides somewhere inside the cloud"""
    P = sheet(n, n).astype(np.float64)
    x, y = P[..., 0] - 0.1, P[..., 1] - 0.17
    P[..., 2] = 2.0 + tilt_x * x + tilt_y * y + 0.5 * (x * x + 0.5 * x * y + 0.8 * y * y)
    return P.astype(np.float32)


COS_EQUAL_ANGLE = 0.00491930224526054         # float32(cos(.)) = 0.9999879, the dot of 12 neighbour pairs of bowl()
DIST_EQUAL = 0.00016779691213741899           # float32(.) * z^2 = |d(p) - d(q)| exactly for a neighbour pair of bowl(3, 1)


def joins():
    """the join comparator at equality and either side of it (tests/test_cloud_hard_cpu.py asserts the equalities).  Every
    segment is a plane (min_inliers 0, curvature limit 1) and nothing is refined, so every join shows in the labels."""
    every = dict(smoothing_size=2, min_inliers=0, max_curvature=1.0, refine=0)
    step = sheet(30, 40, 2.0, 0.0, 0.01)
    step[:, 20:, 2] += F(0.0404)               # more than 0.02 z seen from the near side, less seen from the far side
    return {
        "cos_equal": PlaneCall([bowl()], PlaneParams(angular_threshold=COS_EQUAL_ANGLE, distance_threshold=1.0, **every)),
        "dist_equal": PlaneCall([bowl(3.0, 1.0)], PlaneParams(angular_threshold=1.0, distance_threshold=DIST_EQUAL, **every)),
        "depth_step": PlaneCall([step], PlaneParams(smoothing_size=2, min_inliers=4, refine=0)),
    }


PLANE_SCENES = {"joins": joins, "tall": tall, "snake": snake, "singles": singles, "far": far, "edges": edges, "refine": refine, "many": many}


# ---- cluster scenes -----------------------------------------------------------------------------------------------------------
def box_of(lo, hi):
    """the camera box {x, y, z, height, width, depth} whose crop (expanded by a tenth on every side) holds lo .. hi"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.array([lo[0], lo[1], lo[2], hi[1] - lo[1], hi[0] - lo[0], hi[2] - lo[2]], np.float64)


def box_around(P, margin=0.05):
    good = P[np.isfinite(P).all(axis=1)].astype(np.float64)
    return box_of(good.min(axis=0) - margin, good.max(axis=0) + margin)


def one_box_each(clouds):
    return ClusterCall(clouds, np.stack([box_around(c.reshape(-1, c.shape[-1])[:, :3]) for c in clouds]), np.arange(len(clouds)))


def chain():
    """20 000 points 9 mm apart on a line, one component, in index orders that are bad for a union-find: a root far from
    every member, long hooks"""
    n = 20000
    line = np.zeros((n, 3), np.float32)
    line[:, 0] = (np.arange(n) * 0.009 - 90.0).astype(np.float32)
    line[:, 2] = 1.0
    even_odd = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    orders = {"shuffled": np.random.default_rng(7).permutation(n), "reversed": np.arange(n)[::-1], "even_odd": even_odd}
    return {k: one_box_each([np.ascontiguousarray(line[o])]) for k, o in orders.items()}


def ulps(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


def cell_of(v):
    """the grid cell of a coordinate, as the yardstick and the kernel compute it: floor of the float32 product with 50"""
    return int(np.floor(F(v) * F(50.0)))


def beside_face(m, d):
    """the float32 nearest the face m * 0.02 on the side a step in direction d leaves: the largest value of cell m - 1 for
    d = +1, the smallest value of cell m for d = -1 (the rounding of v * 50 decides, not v itself)"""
    v = ulps(m * 0.02, -8 * d)
    want = m - 1 if d > 0 else m
    assert cell_of(v) == want
    while cell_of(ulps(v, d)) == want:
        v = ulps(v, d)
    return v


DIRECTIONS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def faces():
    """For every one of the 26 directions: a point an ulp before a cell face (a multiple of 0.02) on every axis the direction
    moves along, and a partner across the face at the radius, an ulp inside and an ulp outside; at negative and at positive
    coordinates; the partner before and after the point in index order.  One box per pair; pairs are 0.2 m apart."""
    pts, boxes = [], []
    k = 0
    for sign in (-1.0, 1.0):
        for d in DIRECTIONS:
            for nudge in (-1, 1):
                for partner_first in (False, True):
                    cell = np.array([5 + 10 * (k % 8), 5 + 10 * ((k // 8) % 8), 50 + 10 * (k // 64)], np.float64)
                    k += 1
                    cell = cell if sign > 0 else -cell
                    a = np.zeros(3, np.float32)
                    b = np.zeros(3, np.float32)
                    unit = 0.01 / np.sqrt(float(sum(v * v for v in d)))
                    for ax in range(3):
                        if d[ax] == 0:
                            a[ax] = F(cell[ax] * 0.02 + 0.01)
                            b[ax] = a[ax]
                        else:
                            a[ax] = beside_face(int(cell[ax]), d[ax])       # the last value before the face the direction crosses
                            b[ax] = F(float(a[ax]) + d[ax] * unit)
                    # move the partner along the first moving axis until the pair sits `nudge` ulps from the radius
                    ax = [i for i in range(3) if d[i] != 0][0]
                    def d2(b):
                        dd = a - b
                        return float(F(F(dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]))
                    r2 = float(F(0.01)) * float(F(0.01))
                    for _ in range(64):
                        if d2(b) <= r2:
                            break
                        b[ax] = ulps(b[ax], -d[ax])
                    for _ in range(64):
                        nxt = b.copy()
                        nxt[ax] = ulps(b[ax], d[ax])
                        if d2(nxt) > r2:
                            break
                        b = nxt
                    if nudge > 0:                                           # the first position outside the radius
                        b[ax] = ulps(b[ax], d[ax])
                    pair = [b, a] if partner_first else [a, b]
                    pts += pair
                    lo, hi = np.minimum(a, b).astype(np.float64), np.maximum(a, b).astype(np.float64)
                    boxes.append(box_of(lo - 0.03, hi + 0.03))
    cloud = np.array(pts, np.float32)
    return {"faces": ClusterCall([cloud], np.array(boxes), np.zeros(len(boxes), np.int64))}


def dense():
    """400 exact duplicates and 400 points within 1 mm of them, all in one cell"""
    rng = np.random.default_rng(11)
    base = np.array([0.031, -0.013, 1.249], np.float32)
    P = np.concatenate([np.repeat(base[None], 400, axis=0), base + rng.uniform(-0.0005, 0.0005, (400, 3)).astype(np.float32)])
    return {"dense": one_box_each([P[rng.permutation(800)].astype(np.float32)])}


def clusters_on_a_line(sizes, step=0.004, gap=0.05):
    """len(sizes) clusters along x, points `step` apart inside a cluster, clusters `gap` apart: (points, cluster of each)"""
    pts, who, x = [], [], 0.0
    for k, n in enumerate(sizes):
        for _ in range(n):
            pts.append((x, 0.1 * k, 1.5))
            who.append(k)
            x += step
        x += gap
    return np.array(pts, np.float32), np.array(who)


def ties():
    """clusters of equal size; the one holding the smallest index has its other points last, so it finishes last"""
    out = {}
    for name, sizes in (("2x2", (2, 2)), ("3x2", (2, 2, 2)), ("2x300", (300, 300)), ("3x300", (300, 300, 300)),
                        ("301_300_301", (301, 300, 301))):
        P, who = clusters_on_a_line(sizes)
        last = len(sizes) - 1
        first = np.flatnonzero(who == last)[:1]                     # one point of the last cluster takes index 0 ...
        rest = np.flatnonzero(who == last)[1:]
        order = np.concatenate([first, np.flatnonzero(who != last), rest])        # ... and its others come after everything
        out[name] = one_box_each([np.ascontiguousarray(P[order])])
    return out


def boxes_call(nboxes):
    """a 48-point cloud (six clusters of 3 .. 13 points and single points) under `nboxes` boxes: full, empty-crop, gated (volume
    below 1e-6, NaN, negative extent) and heavily overlapping boxes in a fixed mix"""
    P, who = clusters_on_a_line((13, 11, 8, 7, 5, 3), gap=0.03)
    P = np.concatenate([P, np.array([[0.9, 0.9, 1.5]], np.float32)])
    assert len(P) == 48
    rng = np.random.default_rng(5)
    P = P[rng.permutation(48)]
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    boxes = []
    for i in range(nboxes):
        kind = i % 8
        if kind == 0:
            b = box_of(lo - 0.01, hi + 0.01)                                    # everything
        elif kind == 1:
            b = box_of([5.0, 5.0, 5.0], [5.5, 5.5, 5.5])                        # an empty crop between full ones
        elif kind == 2:
            b = np.array([0.0, 0.0, 1.0, 0.01, 0.01, 0.009])                    # volume 9e-7: gated
        elif kind == 3:
            b = box_of(lo, hi)
            b[i % 6] = np.nan                                                   # NaN: gated
        elif kind == 4:
            b = box_of(lo, hi)
            b[3 + i % 3] = -b[3 + i % 3]                                        # negative extent: gated
        else:                                                                   # overlapping windows sliding along x
            x0 = lo[0] + (hi[0] - lo[0]) * ((i * 37) % 101) / 101.0
            w = 0.03 + 0.01 * (i % 13)
            b = box_of([x0, lo[1] - 0.01, lo[2] - 0.01], [x0 + w, hi[1] + 0.01, hi[2] + 0.01])
        boxes.append(b)
    return ClusterCall([P], np.array(boxes), np.zeros(nboxes, np.int64))


def tiny_crops():
    """calls whose whole crop is 1, 2 and 3 points (bucket tables of 2, 4 and 8 entries), under 40 identical boxes too: every
    box's points alias the same few buckets"""
    out = {}
    P = np.array([[0.0, 0.0, 1.0], [0.005, 0.0, 1.0], [0.5, 0.5, 1.0], [9.0, 9.0, 9.0]], np.float32)
    for n, hi in ((1, [0.001, 0.05, 1.1]), (2, [0.006, 0.05, 1.1]), (3, [0.55, 0.55, 1.1])):
        out["crop_%d" % n] = ClusterCall([P], box_of([-0.02, -0.05, 0.9], hi)[None], np.zeros(1, np.int64))
    # points on the crop's faces exactly (its float32 corners), each with a partner 8 mm inside
    b = box_of([0.1, 0.2, 1.0], [0.112, 0.212, 1.012])
    lo, hi = PointCloudClusterer.cropBox(b)
    Q = np.array([lo, lo + F(0.008) * np.array([1, 0, 0], F), hi - F(0.008) * np.array([0, 1, 0], F), hi,
                  np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))], np.float32)
    out["on_faces"] = ClusterCall([Q], b[None], np.zeros(1, np.int64))
    b = box_of([-0.02, -0.05, 0.9], [0.006, 0.05, 1.1])
    out["crop_2_x40"] = ClusterCall([P], np.repeat(b[None], 40, axis=0), np.zeros(40, np.int64))
    return out


def boxes():
    out = {"300": boxes_call(SELECT_ROUND + 44), "4200": boxes_call(MAX_GRID + 104)}
    out.update(tiny_crops())
    return out


def grid_sheet(n):
    """n points 9 mm apart on a square sheet (row-major), every one inside its box: one component"""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    P = np.stack([(i % side) * 0.009, (i // side) * 0.009, np.full(n, 1.0)], axis=-1).astype(np.float32)
    return P


def crop_edge():
    """all-inside clouds of 65 535, 65 536 and 65 537 cropped points: the host form's first crop capacity exactly, one below
    and one above (the second pass)"""
    return {str(n): one_box_each([grid_sheet(n)]) for n in (HOST_CROP - 1, HOST_CROP, HOST_CROP + 1)}


def chunk_cloud(n):
    """n points far outside the box, except on the first and last index of every 1024-point chunk and on the cloud's last point:
    those lie 8 mm apart inside it"""
    P = np.full((n, 3), 50.0, np.float32)
    P[:, 0] += np.arange(n, dtype=np.float32)
    on = sorted(set([i for i in range(0, n, SCAN_TILE)] + [i for i in range(SCAN_TILE - 1, n, SCAN_TILE)] + [n - 1]))
    for k, i in enumerate(on):
        P[i] = (0.008 * k, 0.0, 1.0)
    return P, on


def chunks():
    out = {}
    box = box_of([-0.01, -0.01, 0.95], [0.2, 0.01, 1.05])
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        out[str(n)] = ClusterCall([chunk_cloud(n)[0]], box[None], np.zeros(1, np.int64))
    big, small = chunk_cloud(5000)[0], chunk_cloud(60)[0]
    out["5000_and_60"] = ClusterCall([big, small], np.stack([box, box, box_around(big), box]), np.array([0, 1, 0, 1]))
    # five floats per point, padded rows: an organized 33 x 31 view of a (33, 40, 5) array
    padded = np.full((33, 40, 5), 77.0, np.float32)
    padded[:, :31, :3] = chunk_cloud(33 * 31)[0].reshape(33, 31, 3)
    out["5_floats_padded"] = ClusterCall([padded[:, :31, :]], box[None], np.zeros(1, np.int64))
    return out


CLUSTER_SCENES = {"chain": chain, "faces": faces, "dense": dense, "ties": ties, "boxes": boxes, "crop_edge": crop_edge,
                  "chunks": chunks}
