"""Every resampling and HOG kernel variant of csrc/pbd_kernels_features.hip on full planes, bit for bit against the oracle.

The variant is chosen from the input alone -- image depth, channel count, the model's sbin, the handle's real type, an
equal-size or a mixed-size call -- so each row of ROWS is one handle and a set of frames; no debug option is involved.  The
frames are tests/hog_hard_frames.py's (saturated gradients, the exact ties of the orientation snap and of the channel pick,
pixels next to a bisector, genuine 16-bit and float ranges, a 2^-30 texture no float holds), at base shapes whose pyramid
levels put the kernels' lanes, windows and tiles at their edges; each test asserts from the handle's own plan that they do.
tests/test_oracle_cpu.py ties the oracle, on the same frames, to float64 / integer statements of the operations."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd._lib import PbdError

import hog_hard_frames as F

pytestmark = pytest.mark.gpu

DEPTHS = {"8U": np.uint8, "16U": np.uint16, "32F": np.float32, "64F": np.float64}
REALS = {"f32": np.float32, "f64": np.float64}
# Base shapes per sbin, rows and cols within 8 sbin .. 200.  The first has the smallest shorter side the pyramid accepts at
# interval 3 (three levels, the last 5 x 5 blocks: 3 x 3 cells); a shorter side of 5 .. 7 sbin, one or two scales, is refused
# by the library as by the oracle (the reference would write past its level array, src/HOGFeatures.cpp:114-118), so no accepted
# pyramid holds an empty feature map -- test_frames_of_less_than_one_octave_are_refused pins that.  The others were searched
# so that the levels of the three together hold the cases check_plan() asserts.
SHAPES = {2: [(37, 16), (183, 56), (110, 67)], 3: [(24, 51), (33, 158), (40, 77)], 4: [(69, 32), (175, 169), (197, 195)],
          5: [(40, 83), (193, 174), (120, 183)], 6: [(101, 48), (155, 168), (185, 89)], 8: [(64, 133), (121, 150), (141, 163)]}
INTERVAL = 3


def model_for(sbin, thresh=1e9):
    """only the front end is under test: two parts, one mixture, 3 x 3 filters, no candidate passes the threshold"""
    return M.synthetic_model(seed=7, pa=[0, 1], nmix=1, ksize=3, sbin=sbin, interval=INTERVAL, thresh=thresh, name="front-end")


def rows_of_the_table():
    rows = [("8U", 3, "f32", 4), ("8U", 3, "f32", 8)]
    rows += [("8U", 3, "f32", s) for s in (2, 3, 5, 6)]
    rows += [("8U", 1, "f32", s) for s in (4, 8, 3, 6)]
    rows += [("8U", cn, "f64", s) for cn in (1, 3) for s in (3, 4, 8)]
    rows += [(d, cn, "f32", s) for d in ("16U", "32F", "64F") for cn in (1, 3) for s in (4, 8, 5)]
    rows += [(d, cn, "f64", s) for d in ("16U", "32F", "64F") for cn in (1, 3) for s in (4, 6)]
    return rows


ROWS = rows_of_the_table()


def row_id(row):
    return "%s-cn%d-%s-sbin%d" % row


def frames_for(depth, cn, shape, seed):
    """name -> frame of the row's depth at `shape`: scene, noise, extremes, vertical, near_bisector, channel_ties (colour) as
    8-bit values in that depth, and for the wider depths the genuine-range frames (64F: with the 2^-30 texture)"""
    IT = DEPTHS[depth]
    out = {name: im.astype(IT) for name, im in F.frames_u8(seed, shape[0], shape[1], cn).items()}
    if IT != np.uint8:
        out.update(F.frames_genuine(IT, seed + 5, shape[0], shape[1], cn))
        assert ("texture" in out) == (depth == "64F")
    assert {"scene", "noise", "extremes", "vertical"} <= set(out) and ("channel_ties" in out) == (cn == 3)
    return out


def check_plan(hd, shapes, sbin, tiled):
    """the cases the compared levels must hold, computed from the handle's plan (change the shape, not the assertion)"""
    lv = []
    for rows, cols in shapes:
        p = hd.plan(rows, cols)
        assert p["nlevels"] >= INTERVAL
        lv += [(int(r), int(c), int(fr), int(fc), l >= INTERVAL) for l, (r, c, fr, fc) in
               enumerate(zip(p["img_rows"], p["img_cols"], p["feat_rows"], p["feat_cols"]))]
    assert any(not down for *_, down in lv) and any(down for *_, down in lv)        # k_resize* and k_pyrdown* levels
    assert {c % 4 for _, c, *_ in lv} == {0, 1, 2, 3}                               # four-pixel lanes, vector loads
    half = (sbin + 1) // 2                  # the block count is rounded up: the window passes the image, the clamp acts
    assert any(c % sbin >= half for _, c, *_ in lv) and any(r % sbin >= half for r, *_ in lv)
    assert any(c % sbin >= half and r % sbin >= half for r, c, *_ in lv)
    assert all(fr >= 3 and fc >= 3 for _, _, fr, fc, _ in lv) and any(min(fr, fc) == 3 for _, _, fr, fc, _ in lv)
    assert any((fr + 2) * (fc + 2) > 256 for _, _, fr, fc, _ in lv)                # more than one workgroup of blocks
    if tiled:
        tr = 16 if sbin <= 4 else 8                                                # hog_tile_rows(sbin), tiles 16 blocks wide
        blk = [(fr + 2, fc + 2) for _, _, fr, fc, _ in lv]
        assert {0, 1, 15} <= {bc % 16 for _, bc in blk}
        assert {0, 1} <= {br % tr for br, _ in blk}
        assert any(br < tr and bc < 16 for br, bc in blk)                          # a level smaller than one tile


def differing(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)))


def compare_planes(tag, imgs_got, imgs_want, feats_got, feats_want):
    assert len(imgs_got) == len(imgs_want) == len(feats_got) == len(feats_want), tag
    for l, (a, b) in enumerate(zip(imgs_got, imgs_want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, l, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"{tag}: image level {l}: {np.count_nonzero(a != b)} of {a.size} elements differ"
    for l, (a, b) in enumerate(zip(feats_got, feats_want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, l, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"{tag}: features level {l}: {np.count_nonzero(a != b)} of {a.size} elements differ"


def resident_planes(hd, frame, rows, cols, cn, IT):
    """level images and feature planes of `frame` of the handle's resident result"""
    p = hd.plan(rows, cols)
    imgs, feats = [], []
    for l in range(p["nlevels"]):
        img = np.empty((int(p["img_rows"][l]), int(p["img_cols"][l]), cn), IT)
        hd.check(hd.lib.pbd_get_pyramid_image(hd.h, frame, l, img.ctypes.data))
        imgs.append(img)
        feats.append(hd.get_stage(_lib.STAGE_FEATURES, frame, l, int(p["feat_rows"][l]), int(p["feat_cols"][l])))
    return imgs, feats


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


_want = {}


def oracle_planes(oracle, flat, T, key, im):
    """the oracle's level images and features of one frame, computed once per (frame, sbin, T) and left unchanged"""
    k = (key, flat.sbin, np.dtype(T).name)
    if k not in _want:
        imgs, _ = oracle.pyramid_images(im, flat.sbin, flat.interval)
        feats, scales = oracle.features_pyramid(flat, im, dtype=T)
        for a in imgs + feats:
            a.flags.writeable = False
        _want[k] = (imgs, feats, scales)
    return _want[k]


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_variant_planes_equal_the_oracle(det_mod, oracle, row):
    depth, cn, real, sbin = row
    IT, T = DEPTHS[depth], REALS[real]
    flat = model_for(sbin).flatten()
    hd = det_mod.Handle(flat, device=0, real_type=_lib.REAL_F32 if T == np.float32 else _lib.REAL_F64)
    try:
        check_plan(hd, SHAPES[sbin], sbin, tiled=(depth == "8U" and cn == 3 and real == "f32" and sbin in (4, 8)))
        eng = det_mod.HOGFeatures(hd)
        for si, shape in enumerate(SHAPES[sbin]):
            for name, im in frames_for(depth, cn, shape, 60 + si).items():
                imgs_want, feats_want, scales = oracle_planes(oracle, flat, T, (name, depth, cn, shape), im)
                feats = eng.pyramid(im)
                assert np.array_equal(eng.scales(), scales)
                imgs = eng.level_images(shape[0], shape[1], cn, IT)
                compare_planes(f"{row_id(row)} {name} {shape}", imgs, imgs_want, feats, feats_want)
    finally:
        hd.close()


@pytest.mark.parametrize("sbin", [3, 4, 8])
def test_frames_of_less_than_one_octave_are_refused(det_mod, oracle, sbin):
    """A shorter side of 5 .. 7 sbin gives one or two scales, fewer than `interval`: the reference would write past
    pyraimages (src/HOGFeatures.cpp:114-118), the library and the oracle refuse; the side the first base shape has is the
    smallest accepted, and one pixel less is refused."""
    hd = det_mod.Handle(model_for(sbin).flatten(), device=0)
    eng = det_mod.HOGFeatures(hd)
    small = min(SHAPES[sbin][0])
    for side in (5 * sbin, 6 * sbin, 7 * sbin, small - 1):
        for shape in ((side, 150), (150, side)):
            with pytest.raises(PbdError) as e:
                eng.pyramid(np.zeros(shape + (3,), np.uint8))
            assert e.value.code == -1
            with pytest.raises(ValueError):
                oracle.pyramid_plan(shape[0], shape[1], sbin, INTERVAL)
    assert hd.plan(small, 150)["nlevels"] == INTERVAL
    hd.close()


# ---- batches --------------------------------------------------------------------------------------------------------------------
def batch_contents(depth, cn, shape, n):
    """n frames of different content at one shape (or, shape a list, one per shape)"""
    shapes = shape if isinstance(shape, list) else [shape] * n
    names = ["scene", "extremes", "vertical", "noise"] if cn == 1 else ["scene", "channel_ties", "vertical", "extremes"]
    out = []
    for i, sh in enumerate(shapes):
        fr = frames_for(depth, cn, sh, 80 + i)
        if depth != "8U" and i == 1:
            out.append(fr["texture" if depth == "64F" else "wide" if depth == "32F" else "full"])
        else:
            out.append(fr[names[i % len(names)]])
    return out


@pytest.mark.parametrize("depth,cn,real,sbin", [("8U", 3, "f32", 4), ("8U", 3, "f32", 8), ("8U", 3, "f32", 3), ("8U", 1, "f32", 4),
                                                ("8U", 3, "f64", 4), ("16U", 3, "f32", 4), ("64F", 1, "f64", 6)],
                         ids=lambda v: str(v))
def test_equal_size_batch_planes_equal_the_oracle(det_mod, oracle, depth, cn, real, sbin):
    """Three equally sized frames of different content in one call (pbd_detect_batch for 8-bit frames, pbd_detect_frames for
    the other depths): the planes of every frame -- the second and third are where the frame index enters the kernels'
    addressing -- equal the oracle's of that frame alone."""
    IT, T = DEPTHS[depth], REALS[real]
    model = model_for(sbin)
    flat = model.flatten()
    shape = SHAPES[sbin][2]
    frames = batch_contents(depth, cn, shape, 3)
    det = det_mod.PartsBasedDetector(device=0, max_batch=3, dtype=T)
    det.distributeModel(model)
    try:
        got = det.detect_batch(frames) if depth == "8U" else det.detect_frames(frames)
        assert got == []
        for f in (1, 2, 0):
            imgs_want, feats_want, _ = oracle_planes(oracle, flat, T, ("batch", depth, cn, shape, f), frames[f])
            imgs, feats = resident_planes(det.hd, f, shape[0], shape[1], cn, IT)
            compare_planes(f"{depth} cn{cn} {real} sbin{sbin} frame {f}", imgs, imgs_want, feats, feats_want)
    finally:
        det.hd.close()


MIXED = [(d, 3 if i % 2 == 0 else 1, r, 4) for i, d in enumerate(("8U", "16U", "32F", "64F")) for r in ("f32", "f64")]
MIXED += [("8U", 1, "f32", 4), ("16U", 1, "f32", 4), ("32F", 3, "f64", 4), ("64F", 3, "f64", 4)]      # the other channel count
MIXED += [("8U", 3, "f32", 8), ("8U", 3, "f32", 3), ("64F", 3, "f64", 8), ("16U", 1, "f32", 3)]


@pytest.mark.parametrize("depth,cn,real,sbin", MIXED, ids=lambda v: str(v))
def test_mixed_size_call_planes_equal_the_oracle(det_mod, oracle, depth, cn, real, sbin):
    """Four frames of different shapes and content in one pbd_detect_frames call (k_resize<PT, Runs>, k_pyrdown<PT, Runs>, the HOG
    kernels over the call's virtual level table): every frame's level images (pbd_get_pyramid_image(h, f, l)) and features
    equal the oracle's of that frame alone, for every depth and both real types."""
    IT, T = DEPTHS[depth], REALS[real]
    model = model_for(sbin)
    flat = model.flatten()
    a, b, c = SHAPES[sbin]
    shapes = [b, a, c, (c[1] // 2 + 11 * sbin, c[0] - 7)]
    frames = batch_contents(depth, cn, shapes, 4)
    assert len({f.shape for f in frames}) == 4
    det = det_mod.PartsBasedDetector(device=0, max_batch=4, dtype=T)
    det.distributeModel(model)
    try:
        assert det.detect_frames(frames) == []
        for f, (im, shape) in enumerate(zip(frames, shapes)):
            imgs_want, feats_want, _ = oracle_planes(oracle, flat, T, ("mixed", depth, cn, shape, f), im)
            imgs, feats = resident_planes(det.hd, f, shape[0], shape[1], cn, IT)
            compare_planes(f"{depth} cn{cn} {real} sbin{sbin} frame {f} {shape}", imgs, imgs_want, feats, feats_want)
    finally:
        det.hd.close()


MANY_SHAPES = [(69, 32), (32, 69), (70, 35), (75, 33)]      # small accepted shapes around SHAPES[4][0], the smallest
MANY = 44                                                    # 44 frames x 3 resized levels = 132 > 128 = _lib.MAX_LEVELS


@pytest.mark.parametrize("depth,cn,real,sbin", [("8U", 3, "f32", 4), ("32F", 1, "f64", 4)], ids=lambda v: str(v))
def test_mixed_call_with_more_levels_than_the_lds_table(det_mod, oracle, depth, cn, real, sbin):
    """One pbd_detect_frames call whose first pyramid launch holds more runs, and whose virtual frame more levels, than the
    kernels' LDS offset table (PBD_MAX_LEVELS): the run search and the level search of every kernel take their global-memory
    branch.  Every frame's level images and features equal the oracle's of that frame alone."""
    IT, T = DEPTHS[depth], REALS[real]
    model = model_for(sbin)
    flat = model.flatten()
    shapes = [MANY_SHAPES[i % len(MANY_SHAPES)] for i in range(MANY)]
    frames = batch_contents(depth, cn, shapes, MANY)
    det = det_mod.PartsBasedDetector(device=0, max_batch=MANY, dtype=T)
    det.distributeModel(model)
    try:
        nlev = [det.hd.plan(*sh)["nlevels"] for sh in shapes]
        assert all(n >= INTERVAL for n in nlev)
        assert sum(min(n, INTERVAL) for n in nlev) > _lib.MAX_LEVELS     # runs of launch 0: every frame's resized levels
        assert sum(nlev) > _lib.MAX_LEVELS                   # levels of the virtual frame
        assert det.detect_frames(frames) == []
        for f, (im, shape) in enumerate(zip(frames, shapes)):
            imgs_want, feats_want, _ = oracle_planes(oracle, flat, T, ("many", depth, cn, shape, f), im)
            imgs, feats = resident_planes(det.hd, f, shape[0], shape[1], cn, IT)
            compare_planes(f"{depth} cn{cn} {real} sbin{sbin} frame {f} {shape}", imgs, imgs_want, feats, feats_want)
    finally:
        det.hd.close()
