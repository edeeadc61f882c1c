"""Portable synthetic inputs (frames and models) for tests and bench.

There is no model or image in the reference tree (``models/`` is an empty git submodule, SURVEY.md
section 0), so every input is generated here.  The generators use a counter-based splitmix64 stream
and integer / exactly-representable float64 arithmetic only (no libm calls), so the same seed gives
bit-identical arrays on every machine -- required because golden fixtures are produced in the build
container and re-checked on the GPU box.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1


def splitmix64(seed: int, n: int, stream: int = 0) -> np.ndarray:
    """n 64-bit outputs of splitmix64 started at ``seed`` (counter based, vectorised)."""
    with np.errstate(over="ignore"):
        base = np.uint64((seed * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03 + 0x1234567) & _M64)
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = base + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform_u32(seed: int, n: int, stream: int = 0) -> np.ndarray:
    return (splitmix64(seed, n, stream) >> np.uint64(32)).astype(np.int64)


def randint(seed: int, n: int, lo: int, hi: int, stream: int = 0) -> np.ndarray:
    """integers in [lo, hi] (inclusive); tiny modulo bias is irrelevant here."""
    return lo + (uniform_u32(seed, n, stream) % (hi - lo + 1))


def normalish(seed: int, n: int, stream: int = 0) -> np.ndarray:
    """Approximately N(0,1) float64 values: Irwin-Hall sum of 12 uniform 16-bit integers.

    Exact integer sums, one exact scaling -> bit-identical everywhere."""
    raw = splitmix64(seed, 3 * n, stream).reshape(n, 3)
    acc = np.zeros(n, dtype=np.int64)
    for k in range(3):
        w = raw[:, k]
        for s in (0, 16, 32, 48):
            acc += ((w >> np.uint64(s)) & np.uint64(0xFFFF)).astype(np.int64)
    # 12 uniforms on [0, 65535]: mean 12*32767.5, variance 12*(65536^2-1)/12
    return (acc.astype(np.float64) - 393210.0) / 65536.0


def synthetic_frame(seed: int, rows: int = 480, cols: int = 640, channels: int = 3, kind: str = "scene") -> np.ndarray:
    """uint8 frame (rows, cols, channels), BGR interleaved when channels == 3.

    kind = "scene": smooth background (integer bilinear up-sampling of a 1/16-resolution random
    grid) + 8 random filled rectangles + +-8 uniform noise;
    "noise": uniform noise; "constant": all 128."""
    if kind == "constant":
        return np.full((rows, cols, channels), 128, dtype=np.uint8)
    if kind == "noise":
        v = uniform_u32(seed, rows * cols * channels, stream=7) & 0xFF
        return v.reshape(rows, cols, channels).astype(np.uint8)
    gr, gc = rows // 16 + 2, cols // 16 + 2
    grid = (uniform_u32(seed, gr * gc * channels, stream=1) & 0xFF).reshape(gr, gc, channels)
    y = np.arange(rows, dtype=np.int64)
    x = np.arange(cols, dtype=np.int64)
    y0, fy = y // 16, (y % 16)[:, None, None]
    x0, fx = x // 16, (x % 16)[None, :, None]
    g00 = grid[y0][:, x0]
    g01 = grid[y0][:, x0 + 1]
    g10 = grid[y0 + 1][:, x0]
    g11 = grid[y0 + 1][:, x0 + 1]
    img = ((16 - fy) * ((16 - fx) * g00 + fx * g01) + fy * ((16 - fx) * g10 + fx * g11) + 128) >> 8
    rect = uniform_u32(seed, 8 * (4 + channels), stream=2).reshape(8, 4 + channels)
    for r in rect:
        ry, rx = int(r[0] % rows), int(r[1] % cols)
        rh, rw = 8 + int(r[2] % max(rows // 3, 1)), 8 + int(r[3] % max(cols // 3, 1))
        img[ry:ry + rh, rx:rx + rw, :] = (r[4:4 + channels] & 0xFF)[None, None, :]
    noise = (uniform_u32(seed, rows * cols * channels, stream=3) % 17) - 8
    img = img + noise.reshape(rows, cols, channels)
    return np.clip(img, 0, 255).astype(np.uint8)


# 1-based parent table of the 26-part person tree (parent < child as asserted
# in matlab/detection/detect_fast.m:76)
PERSON_PA = [0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10, 11, 12, 13, 2, 15, 16, 17, 18, 15, 20, 21, 22, 23, 24, 25]


def synthetic_depth(seed: int, rows: int = 480, cols: int = 640, dtype=np.uint16, holes: bool = True, inf: bool = False) -> np.ndarray:
    """Deterministic depth image (rows, cols) of `dtype` (uint8, uint16, float32 or float64) for the 3-D box stage.

    A tilted background plane (millimetres, about 2-4 m), 6 nearer blobs (rectangles at 0.6-1.8 m with a gentle slope of their
    own), +-3 mm noise; with `holes`, 24 rectangles of missing depth (0), and for the float types NaN in every other hole;
    with `inf`, a few pixels of +Inf and -Inf (float types only).  Float images hold metres (millimetres / 1000, one correctly
    rounded division).  Integer arithmetic otherwise, so the same seed gives the same image everywhere."""
    dtype = np.dtype(dtype)
    y = np.arange(rows, dtype=np.int64)[:, None]
    x = np.arange(cols, dtype=np.int64)[None, :]
    prm = randint(seed, 4, 0, 1000, stream=11)
    z = 2000 + prm[0] + ((y * (1 + prm[1] % 3) * 1000) // max(rows, 1)) + ((x * (prm[2] % 5)) * 200) // max(cols, 1)
    z = np.broadcast_to(z, (rows, cols)).copy()
    blob = uniform_u32(seed, 6 * 6, stream=12).reshape(6, 6)
    for b in blob:
        by, bx = int(b[0] % rows), int(b[1] % cols)
        bh, bw = 4 + int(b[2] % max(rows // 3, 1)), 4 + int(b[3] % max(cols // 4, 1))
        near = 600 + int(b[4] % 1200)
        slope = int(b[5] % 7) - 3
        yy = np.arange(by, min(by + bh, rows), dtype=np.int64)[:, None]
        z[by:by + bh, bx:bx + bw] = near + slope * (yy - by)
    z = z + (uniform_u32(seed, rows * cols, stream=13) % 7 - 3).reshape(rows, cols)
    hole = np.zeros((rows, cols), np.int8)
    if holes:
        hr = uniform_u32(seed, 24 * 4, stream=14).reshape(24, 4)
        for k, r in enumerate(hr):
            hy, hx = int(r[0] % rows), int(r[1] % cols)
            hh, hw = 1 + int(r[2] % max(rows // 12, 1)), 1 + int(r[3] % max(cols // 12, 1))
            hole[hy:hy + hh, hx:hx + hw] = 1 + (k & 1)
    if dtype == np.uint8:
        out = np.clip(z // 16, 1, 255).astype(np.uint8)
    elif dtype == np.uint16:
        out = np.clip(z, 1, 65535).astype(np.uint16)
    elif dtype in (np.float32, np.float64):
        out = (z.astype(np.float64) / 1000.0).astype(dtype)
    else:
        raise ValueError(f"depth dtype {dtype}: uint8, uint16, float32 or float64")
    out[hole == 1] = 0
    if dtype.kind == "f":
        out[hole == 2] = np.nan
        if inf:
            pts = uniform_u32(seed, 16, stream=15)
            for k in range(8):
                out[int(pts[2 * k] % rows), int(pts[2 * k + 1] % cols)] = np.inf if k & 1 else -np.inf
    else:
        out[hole == 2] = 0
    return out
