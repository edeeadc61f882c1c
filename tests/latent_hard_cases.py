"""Built inputs for the four kernels of csrc/pbd_kernels_examples.hip (k_latent_mask, k_latent_best, k_ex_walk, k_ex_gather) and,
cached per process, the yardstick's results on them (tests/test_latent_hard_cpu.py, tests/test_gpu_latent_hard.py,
tests/test_gpu_examples_hard.py).

Builders only: numpy and the oracle, no handle, no randomness beyond fixed seeds, so every machine builds the same inputs.  What
each case is built to reach is asserted from the yardstick alone in tests/test_latent_hard_cpu.py.

A latent case is one pbd_detect_latent call: the model, the frames, per frame the part boxes (x1, y1, x2, y2 inclusive) and the
fixed mixtures (or None), and the overlap AS THE CALL TAKES IT, a float32.  include/pbd.h: the test is made in double, strictly
greater, against that float widened, so the yardstick is given float(np.float32(overlap)), never the decimal it was written as.

The sizes named here restate constants of the kernels: a case that crosses one of them says which.
"""
import functools
from collections import namedtuple

import numpy as np

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import synth

MASK_GRID = 65536        # launch_latent_mask: at most this many blocks ...
MASK_THREADS = 256       # ... of this many threads, one response value each per round; also the threads of k_latent_best
GATHER_GRID = 8192       # kExMaxGrid: at most this many blocks of k_ex_gather ...
GATHER_WAVES = 4         # ... of kExGatherWaves wavefronts, one (record, part) pair each per round
GATHER_RECORDS = 1300    # records of the person model (26 parts) that make k_ex_gather go round twice

LOW = -100.0             # a threshold every root passes

LatentCase = namedtuple("LatentCase", "model frames boxes overlap mixtures")


def widened(overlap) -> float:
    """the double the kernel compares with: the call's float32 widened"""
    return float(np.float32(overlap))


# ---- models ---------------------------------------------------------------------------------------------------------------
def tiny():
    return M.synthetic_tiny_model(thresh=LOW)


SIZES = {"1_3_6": (2, [1, 3, 6]), "9_12_5": (3, [9, 12, 5]), "1": (2, [1]), "5": (2, [5])}


@functools.lru_cache(maxsize=None)
def sizes_model(name):
    """4 parts (one of them a grandchild) whose filter sizes cycle through the list over the mixtures of a part: 1_3_6 has the
    sizes (1, 3) (6, 1) (3, 6) (1, 3), 9_12_5 has (9, 12, 5) in every part, 1 has 1 x 1 filters only, 5 has 5 x 5 filters
    only (the one size PBD_CONV_MFMA takes)"""
    nmix, ksize = SIZES[name]
    return M.synthetic_model(seed=40 + nmix, pa=[0, 1, 1, 2], nmix=nmix, ksize=ksize, interval=5, thresh=LOW, name="sizes_" + name)


def sizes_frame():
    return synth.synthetic_frame(31, 140, 120)


def ties_model():
    """the tiny model with its component twice and channel 31 of every filter 0: on a frame of one colour every feature the
    HOG stage writes is 0 and the border's 1 on channel 31 meets a 0 weight, so every response is exactly 0"""
    m = M.synthetic_tiny_model(thresh=LOW)
    for f in m.filtersw:
        f.reshape(f.shape[0], f.shape[0], m.flen)[:, :, m.flen - 1] = 0.0
    for tab in (m.filterid, m.biasid, m.defid):
        tab.append([list(x) for x in tab[0]])
    m.parentid.append(list(m.parentid[0]))
    m.validate()
    return m


def flat_frame(rows, cols, value=90):
    return np.full((rows, cols, 3), value, np.uint8)


def best_boxes(model, im):
    """the part boxes (inclusive corners) of the oracle's best detection of im"""
    from oracle import oracle
    best = max(oracle.detect(model.flatten(), im), key=lambda r: r["score"])
    return [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best["parts"]]


# ---- the latent cases -----------------------------------------------------------------------------------------------------
HALF_BOX = (8, 8, 27, 47)            # 20 x 40: a 20 x 20 rectangle wholly inside has IoU 400 / 800
TENTHS_BOX = (12, 15, 31, 28)        # 20 x 14 inside one 20 x 20 rectangle: IoU 280 / 400
TIES_BOX = (10, 10, 80, 60)
TIES_LOW_BOX = (10, 42, 80, 92)      # the same, 8 cells further down: the first maximum is beyond the first round of 256 threads
INT32_BOX = (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0))


def _tiny_case(box, overlap):
    return LatentCase(tiny(), [synth.synthetic_frame(5, 72, 96)], [[box] * 3], np.float32(overlap), None)


def sizes_case(name, overlap=0.5, mixtures=None, boxes=None):
    m, im = sizes_model(name), sizes_frame()
    return LatentCase(m, [im], [best_boxes(m, im) if boxes is None else boxes], np.float32(overlap), mixtures)


def _mixtures_fixed():
    """frame 0: every part fixed, to the mixtures of the free search's own arg-max placement (so the fixed search finds it
    again); frame 1: parts 1 and 3 fixed, 0 and 2 free"""
    m = sizes_model("9_12_5")
    frames = [sizes_frame(), synth.synthetic_frame(32, 100, 132)]
    boxes = [best_boxes(m, f) for f in frames]
    free = latent_stages(m, frames[0], boxes[0], widened(0.4))
    return LatentCase(m, frames, boxes, np.float32(0.4), [[mix for (_, _, mix) in free["placement"]["argmax"]], [-1, 1, -1, 0]])


def _mixtures_never():
    """part 1 of 1_3_6 has a 6 x 6 and a 1 x 1 filter; its box is the 6 x 6 rectangle of the best detection enlarged to 40 x 40
    pixels, and it is fixed to the 1 x 1 mixture, whose rectangle is one cell of at most 21 x 21 pixels: IoU at most 441 / 1600"""
    m, im = sizes_model("1_3_6"), sizes_frame()
    boxes = best_boxes(m, im)
    x1, y1 = boxes[1][0], boxes[1][1]
    boxes[1] = (x1, y1, x1 + 39, y1 + 39)
    return LatentCase(m, [im], [boxes], np.float32(0.5), [[-1, 1, -1, -1]])


def _ties_mixed():
    """the flat frame as frame 1 of three of different sizes"""
    m = ties_model()
    frames = [synth.synthetic_frame(41, 64, 80), flat_frame(72, 96), synth.synthetic_frame(42, 50, 130)]
    return LatentCase(m, frames, [[TIES_BOX] * 3, [TIES_LOW_BOX] * 3, [TIES_BOX] * 3], np.float32(0.1), None)


LATENT_CASES = {
    "half": lambda: _tiny_case(HALF_BOX, 0.5),
    "below_half": lambda: _tiny_case(HALF_BOX, BELOW_HALF),
    "seven_tenths": lambda: _tiny_case(TENTHS_BOX, 0.7),
    "sizes_1_3_6": lambda: sizes_case("1_3_6"),
    "sizes_9_12_5": lambda: sizes_case("9_12_5"),
    "mixtures_fixed": _mixtures_fixed,
    "mixtures_never": _mixtures_never,
    "ties": lambda: LatentCase(ties_model(), [flat_frame(72, 96)], [[TIES_BOX] * 3], np.float32(0.1), None),
    "ties_mixed": _ties_mixed,
    "keep_all": lambda: sizes_case("1_3_6", -1.0),
    "keep_none": lambda: sizes_case("1_3_6", np.inf),
    "int32_box": lambda: sizes_case("9_12_5", 0.0, boxes=[INT32_BOX] * 4),
}
BOTH_WALKS = ("sizes_1_3_6", "sizes_9_12_5", "ties", "ties_mixed")


@functools.lru_cache(maxsize=None)
def latent_case(name):
    return LATENT_CASES[name]()


# ---- the yardstick of a latent call, stage by stage ----------------------------------------------------------------------------
def latent_stages(model, im, boxes, overlap, mixtures=None, dtype=np.float32):
    """examples.latent_search with every stage kept: dict(feats, scales, resp [level] (totmix, H, W) masked, rootv / rooti
    [level] (NC, H, W), level, component, root_x, root_y, score (T), found, placement {walk: [(x, y, mixture)]}, parts {walk:
    (nparts, 4) x, y, w, h}).  The best root is the first maximum in (level, component, y, x) order."""
    from oracle import oracle
    uflat = E.unique_model(model).flatten()
    feats, scales = oracle.features_pyramid(uflat, im, dtype)
    out = {"uflat": uflat, "feats": feats, "scales": scales, "resp": [], "rootv": [], "rooti": []}
    best, maps = None, None
    for lvl, feat in enumerate(feats):
        resp = E.mask_responses(uflat, oracle.responses(uflat, feat), scales[lvl], boxes, overlap, mixtures, dtype)
        dps = [oracle.dp_min(uflat, c, resp) for c in range(uflat.ncomponents)]
        out["resp"].append(resp)
        out["rootv"].append(np.stack([d[3] for d in dps]))
        out["rooti"].append(np.stack([d[4] for d in dps]).astype(np.int32))
        for c, (Ix, Iy, Ik, rootv, rooti) in enumerate(dps):
            i = int(np.argmax(rootv))       # first maximum in raster order
            if best is None or rootv.flat[i] > best[0]:
                best = (rootv.flat[i], lvl, c, i % rootv.shape[1], i // rootv.shape[1])
                maps = (Ix, Iy, Ik, rooti)
    v, lvl, c, x, y = best
    IxRaw, IyRaw, Ik, _, rooti = E.raw_maps(uflat, c, out["resp"][lvl])
    out["placement"] = {"reference": E.walk(uflat, c, x, y, *maps),
                        "argmax": E.walk(uflat, c, x, y, IxRaw, IyRaw, Ik, rooti, argmax=True)}
    out["parts"] = {}
    for walk, pl in out["placement"].items():
        parts = []
        for p, (px, py, m) in enumerate(pl):
            gm = int(uflat.mix_offset[uflat.part_offset[c] + p]) + m
            x1, y1, x2, y2 = E.part_rects(px, py, int(uflat.filter_ksize[uflat.filterid[gm]]), scales[lvl], dtype)
            parts.append((int(x1), int(y1), int(x2 - x1), int(y2 - y1)))
        out["parts"][walk] = np.asarray(parts, np.int32)
    out.update(level=lvl, component=c, root_x=x, root_y=y, score=v, found=float(np.float32(v)) > -5e9)
    return out


@functools.lru_cache(maxsize=None)
def latent_yardstick(name, dtype_name="float32"):
    """[latent_stages of frame f] of a case"""
    case = latent_case(name)
    dtype = np.dtype(dtype_name).type
    return [latent_stages(case.model, im, case.boxes[f], widened(case.overlap), None if case.mixtures is None else case.mixtures[f],
                          dtype) for f, im in enumerate(case.frames)]


def root_offset(st, lvl, c, x, y):
    """the offset of a root score in its frame's range as k_latent_best scans it: levels in order, each (component, y, x)"""
    off = sum(int(r.size) for r in st["rootv"][:lvl])
    _, H, W = st["rootv"][lvl].shape
    return off + (c * H + y) * W + x


# ---- built records for pbd_examples* --------------------------------------------------------------------------------------------
def map_points(rows, cols):
    """(x, y): the four corners, the four edge midpoints and the centre of a rows x cols map"""
    xs, ys = (0, cols // 2, cols - 1), (0, rows // 2, rows - 1)
    return [(x, y) for y in ys for x in xs]


def record_rows(stride, entries, frame_offset=0):
    """(n, stride) int32 records of (frame, component, level, x, y) entries: the five words pbd_examples* read"""
    rec = np.zeros((len(entries), stride), np.int32)
    for i, (f, c, l, x, y) in enumerate(entries):
        rec[i, :5] = (f + frame_offset, c, l, x, y)
    return rec


def built_entries(flat, shapes):
    """levels 0, middle and last of a pyramid of map `shapes`, every component, map_points"""
    n = len(shapes)
    return [(0, c, l, x, y) for l in (0, n // 2, n - 1) for c in range(flat.ncomponents) for (x, y) in map_points(*shapes[l])]


@functools.lru_cache(maxsize=None)
def frame_maps(kind, name, dtype_name="float32"):
    """the oracle's maps of a frame of a model, shared by the tests of one process: ("sizes", name) or ("person", "120x160")"""
    dtype = np.dtype(dtype_name).type
    if kind == "sizes":
        return E.FrameMaps(sizes_model(name).flatten(), sizes_frame(), dtype)
    return E.FrameMaps(M.synthetic_person_model(thresh=LOW).flatten(), person_frame(), dtype)


def person_frame():
    return synth.synthetic_frame(2, 120, 160)


def level_shapes(fm):
    return [(f.shape[0], f.shape[1] // E.FLEN) for f in fm.feats]


def seeded_positions(shapes, n, seed=7):
    """n of the (level, x, y) root positions of a pyramid, seeded, in a shuffled order"""
    every = [(l, x, y) for l, (rows, cols) in enumerate(shapes) for y in range(rows) for x in range(cols)]
    pick = np.random.default_rng(seed).permutation(len(every))[:n]
    return len(every), [every[i] for i in pick]


# bad records in a mixed plan: frames of three sizes, frame_offset 5
BAD_FRAMES = ((64, 80), (96, 72), (50, 130))
BAD_OFFSET = 5


def bad_model():
    return M.synthetic_face_model(nparts=7, ncomponents=3, thresh=LOW)


def bad_frames():
    return [synth.synthetic_frame(3 + k, r, c) for k, (r, c) in enumerate(BAD_FRAMES)]


def bad_entries(nlevels, shapes, NC):
    """[(entry, reason or None)]: good records interleaved with one bad record per reason; nlevels[f], shapes[f][l] = (rows,
    cols).  The level reason names frame 0's own level count, a level that the taller pyramid of frame 1 has: in the plan's table
    of virtual levels it is frame 1's level 0."""
    short, tall = 0, int(np.argmax(nlevels))
    assert nlevels[short] < nlevels[tall]
    ls = nlevels[short]
    r0, c0 = shapes[0][1]
    bad = [((-1, 0, 0, 0, 0), "frame below 0"),
           ((len(nlevels), 0, 0, 0, 0), "frame at nframes"),
           ((1, 1, -1, 0, 0), "level below 0"),
           ((short, 0, ls, 0, 0), "level at this frame's own count"),
           ((0, -1, 1, 1, 1), "component -1"),
           ((2, NC, 0, 1, 1), "component NC"),
           ((0, 2, 1, -1, 0), "root x -1"),
           ((0, 1, 1, 0, r0), "root y at rows")]
    out = []
    for k, b in enumerate(bad):
        f = k % len(nlevels)
        l = k % nlevels[f]
        rows, cols = shapes[f][l]
        out.append(((f, k % NC, l, (3 * k) % cols, (5 * k) % rows), None))
        out.append(b)
    f = tall
    out.append(((f, 0, nlevels[f] - 1, shapes[f][-1][1] - 1, shapes[f][-1][0] - 1), None))
    return out


# ---- exact arithmetic for the conditions ----------------------------------------------------------------------------------------
def exact_iou(x, y, k, scale, box, dtype=np.float32):
    """the IoU of the record rectangle of a part of size k at (x, y) with box, as a fractions.Fraction of integers"""
    from fractions import Fraction
    x1, y1, x2, y2 = (int(v) for v in E.part_rects(x, y, k, scale, dtype))
    iw = max(0, min(x2, box[2]) - max(x1, box[0]) + 1)
    ih = max(0, min(y2, box[3]) - max(y1, box[1]) + 1)
    area, barea = (x2 - x1 + 1) * (y2 - y1 + 1), (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
    return Fraction(iw * ih, area + barea - iw * ih)


def positions_with_iou(shape, k, scale, box, value):
    rows, cols = shape
    return [(x, y) for y in range(rows) for x in range(cols) if exact_iou(x, y, k, scale, box) == value]


def plan_maps(plan, sbin=4):
    """[(rows, cols)] of the feature maps of oracle.pyramid_plan's level images"""
    from oracle import oracle
    return [oracle.hog_dims(int(r), int(c), sbin) for r, c in zip(plan[0], plan[1])]
