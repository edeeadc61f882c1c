"""Synthetic organized clouds for the plane-removal tests (tests/test_planes_cpu.py, tests/test_gpu_planes.py): depth images
built from closed forms, back-projected with pointcloud.cloud_from_depth.  No randomness, so every machine builds the same
clouds."""
import numpy as np

from partsbaseddetector_amd.pointcloud import PinholeCamera, cloud_from_depth


def camera(rows: int, cols: int, cy: float = 0.5) -> PinholeCamera:
    f = 525.0 * cols / 640.0
    return PinholeCamera(f, f, cols / 2.0 - 0.5, rows * cy - 0.5)

BALL = (0.0, 1.0 - 0.2 - 0.03, 1.6, 0.2)          # the room's ball: centre x, y, z and radius (m), 3 cm above the floor


def rays(rows: int, cols: int, cam: PinholeCamera):
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy


def room(rows: int = 480, cols: int = 640, holes: bool = True, ball: bool = True):
    """a floor 1 m below the camera (principal point in the upper fifth of the view), a wall at 3 m, two boxes standing on the
    floor (their front faces are planes, their edges depth jumps), a ball (BALL) just above the floor (not a plane), and NaN
    and zero holes"""
    cam = camera(rows, cols, 0.2)
    rx, ry = rays(rows, cols, cam)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(ry > 0, 1.0 / ry, np.inf)
    d = np.minimum(d, 3.0)
    for x0, x1, z, top in ((-0.9, -0.45, 2.4, 0.45), (0.35, 0.8, 2.0, 0.5)):
        face = (rx * z >= x0) & (rx * z <= x1) & (ry * z >= top) & (ry * z <= 1.0)
        d = np.where(face & (z < d), z, d)
    if ball:
        cx, cy, cz, r = BALL
        a = rx * rx + ry * ry + 1.0                       # |ray|^2, ray = (rx, ry, 1)
        b = -2.0 * (rx * cx + ry * cy + cz)
        c = cx * cx + cy * cy + cz * cz - r * r
        disc = b * b - 4 * a * c
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / (2 * a)
        hit = (disc > 0) & (t > 0) & (t < d)
        d = np.where(hit, t, d)
    if holes:
        d[rows // 5:rows // 5 + rows // 40, cols // 2:cols // 2 + cols // 30] = np.nan
        d[rows - rows // 8:rows - rows // 8 + 3, cols // 6:cols // 3] = 0.0
    return cloud_from_depth(d.astype(np.float32), cam), cam


def tilted(rows: int = 240, cols: int = 320):
    """one tilted plane 0.4 x + 0.25 y + z = 2.5 across the whole view, with a hole"""
    cam = camera(rows, cols)
    rx, ry = rays(rows, cols, cam)
    d = 2.5 / (0.4 * rx + 0.25 * ry + 1.0)
    d[rows // 3:rows // 3 + 12, cols // 3:cols // 3 + 20] = np.nan
    return cloud_from_depth(d.astype(np.float32), cam), cam


def patches(rows: int = 120, cols: int = 400):
    """flat patches at 2 m on NaN: the first gives a segment of exactly 1000 points (25 x 40 centres with a valid window),
    the second one of 1001 (7 x 143); s = 5, so a patch of h x w pixels has (h - 12) x (w - 12) such centres"""
    cam = camera(rows, cols)
    d = np.full((rows, cols), np.nan)
    d[5:5 + 37, 5:5 + 52] = 2.0
    d[60:60 + 19, 100:100 + 155] = 2.0
    return cloud_from_depth(d.astype(np.float32), cam), cam


def bent(rows: int, cols: int, radius: float):
    """a cylinder section of the given radius (m) around a vertical axis, 2 m ahead: one segment whose curvature falls with
    the radius"""
    cam = camera(rows, cols)
    rx, _ = rays(rows, cols, cam)
    # the ray (rx, ry, 1) t meets x^2 + (z - (2 + R))^2 = R^2, the near side
    zc = 2.0 + radius
    a = rx * rx + 1.0
    b = -2.0 * zc
    c = zc * zc - radius * radius
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)
    return cloud_from_depth(t.astype(np.float32), cam), cam
