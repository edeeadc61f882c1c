"""Built inputs for the scale NMS (pbd_set_scale_nms, pbd_scale_nms, scalenms.py; include/pbd.h states the rule).

  record lists   RECORD_CASES: (name, rows, dl, hand-worked kept indices); a row is (frame, level, component, score, x, y, w, h)
  plane frames   plane_frames(): built pyramids of random stepped planes (many exact ties) with roots of different filter sides,
                 several components, a pad of (2, 2), a fine octave's longer level list and an empty level
  oracle frames  frame_levels(): the root planes of a real frame from the CPU oracle; the detect path's inputs of
                 test_gpu_scale_nms.py, whose conditions test_scale_nms_cpu.py checks
  mutants        keep_mutant(): the all-pairs rule with one clause changed
"""
import numpy as np

from partsbaseddetector_amd import scalenms as S

DLS = (0, 1, 2, 5)
SHAPES = ((48, 64), (96, 128))
NAN = float("nan")

# (frame, level, component, score, x, y, w, h)
A = (0, 3, 0, 1.0, 0, 0, 10, 10)          # the rectangle most cases measure against: centre (10, 10) doubled
RECORD_CASES = (
    # b's doubled centre exactly on a's left edge (2 x_a = 0): inside.  a's centre is not in b
    ("edge_inclusive", [A, (0, 3, 0, 2.0, -2, 3, 4, 4)], 0, [1]),
    # b's doubled centre exactly on a's right edge (2 (x_a + w_a) = 20): outside
    ("edge_exclusive", [A, (0, 3, 0, 2.0, 8, 3, 4, 4)], 0, [0, 1]),
    ("edge_exclusive_y", [A, (0, 3, 0, 2.0, 3, 8, 4, 4)], 0, [0, 1]),
    # a rectangle without width covers nothing, but its centre can be covered: the better one, b, has w = 0
    ("zero_width_covers_nothing", [(0, 3, 0, 1.0, 4, 4, 2, 2), (0, 3, 0, 2.0, 5, 3, 0, 4)], 0, [1]),
    ("zero_width_both", [(0, 3, 0, 1.0, 5, 5, 0, 0), (0, 3, 0, 2.0, 5, 5, 0, 0)], 0, [0, 1]),
    ("negative_width", [(0, 3, 0, 1.0, 9, 9, -4, 4), (0, 3, 0, 2.0, 5, 5, -4, -4)], 0, [0, 1]),
    # odd width: the doubled centre 2 * 2 + 1 = 5 is no pixel; 0 <= 5 < 10
    ("odd_width", [(0, 3, 0, 1.0, 0, 0, 5, 5), (0, 3, 0, 2.0, 2, 2, 1, 1)], 0, [1]),
    ("even_width", [(0, 3, 0, 1.0, 0, 0, 4, 4), (0, 3, 0, 2.0, 3, 3, 2, 2)], 0, [0, 1]),   # centre 8 = 2 (0 + 4): outside; a's 4 < 6
    # only covers(small, ...) fails: the small better one lies inside the large one, away from its centre
    ("small_inside_large", [(0, 3, 0, 1.0, 0, 0, 40, 40), (0, 4, 0, 2.0, 30, 30, 4, 4)], 1, [1]),
    ("large_over_small", [(0, 3, 0, 2.0, 0, 0, 40, 40), (0, 4, 0, 1.0, 30, 30, 4, 4)], 1, [0]),
    # level distance: exactly dl apart is near, dl + 1 is not
    ("level_at_dl", [(0, 1, 0, 1.0, 0, 0, 10, 10), (0, 3, 0, 2.0, 1, 1, 10, 10)], 2, [1]),
    ("level_beyond_dl", [(0, 1, 0, 1.0, 0, 0, 10, 10), (0, 4, 0, 2.0, 1, 1, 10, 10)], 2, [0, 1]),
    ("dl_zero_other_level", [(0, 1, 0, 1.0, 0, 0, 10, 10), (0, 2, 0, 2.0, 0, 0, 10, 10)], 0, [0, 1]),
    ("dl_all_levels", [(0, 0, 0, 1.0, 0, 0, 10, 10), (0, 200, 0, 2.0, 0, 0, 10, 10)], 255, [1]),
    # the own plane and other components take part
    ("own_plane", [(0, 3, 0, 2.0, 0, 0, 10, 10), (0, 3, 0, 1.0, 1, 0, 10, 10)], 0, [0]),
    ("other_component", [(0, 3, 0, 1.0, 0, 0, 10, 10), (0, 3, 1, 2.0, 1, 0, 12, 12)], 0, [1]),
    # ties go to the earlier record; +0.0 and -0.0 tie
    ("tie_earlier_wins", [(0, 3, 0, 1.5, 0, 0, 10, 10), (0, 4, 0, 1.5, 0, 0, 10, 10)], 1, [0]),
    ("tie_of_zeros", [(0, 3, 0, -0.0, 0, 0, 10, 10), (0, 3, 1, 0.0, 0, 0, 10, 10)], 0, [0]),
    # a local-maximum rule: the middle one is beaten by the last, the first by the middle one although that one is dropped
    ("chain", [(0, 3, 0, 1.0, 0, 0, 10, 10), (0, 3, 0, 2.0, 4, 0, 10, 10), (0, 3, 0, 3.0, 8, 0, 10, 10)], 0, [2]),
    # frames do not meet; a NaN score is never kept and beats nobody
    ("frames_apart", [(0, 3, 0, 1.0, 0, 0, 10, 10), (1, 3, 0, 2.0, 0, 0, 10, 10), (4, 3, 0, 3.0, 0, 0, 10, 10)], 5, [0, 1, 2]),
    ("nan_score", [(0, 3, 0, 1.0, 0, 0, 10, 10), (0, 3, 0, NAN, 0, 0, 10, 10), (0, 3, 0, 0.5, 1, 1, 10, 10)], 0, [0]),
    ("inf_scores", [(0, 3, 0, np.inf, 0, 0, 10, 10), (0, 3, 0, np.inf, 0, 0, 10, 10), (0, 3, 0, -np.inf, 0, 0, 10, 10)], 0, [0]),
)


def record_list(rows, stride=12, frame_offset=0):
    """the records (n, stride) int32 of RECORD_CASES rows: nparts 1, the rectangle as part 0, every unused word distinct"""
    out = np.zeros((len(rows), stride), np.int32)
    for i, (f, l, c, s, x, y, w, h) in enumerate(rows):
        r = np.arange(stride, dtype=np.int32) + 1000 * (i + 1)
        r[:5] = (f + frame_offset, c, l, x // 4, y // 4)
        r[5] = np.array([s], np.float32).view(np.int32)[0]
        r[6], r[7] = 1, 0
        r[8:12] = (x, y, w, h)
        out[i] = r
    return out


def random_records(n, nframes, seed, stride=12, span=60, nlevels=8):
    """n records over nframes frames: rectangles of a few sizes at random places, scores with many ties, a few NaN"""
    rng = np.random.default_rng(seed)
    frames = np.sort(rng.integers(0, nframes, n))
    rows = []
    for f in frames:
        w = int(rng.choice([0, 5, 8, 12, 20]))
        s = float(np.round(rng.standard_normal() * 3) / 2)
        rows.append((int(f), int(rng.integers(0, nlevels)), int(rng.integers(0, 3)), NAN if rng.random() < 0.04 else s,
                     int(rng.integers(-10, span)), int(rng.integers(-10, span)), w, w))
    return record_list(rows, stride)


# ---- mutants of the rule -----------------------------------------------------------------------------------------------------
MUTATIONS = ("closed_interval", "one_direction", "greater_equal", "tie_to_later", "own_plane_excluded", "level_less_than_dl")


def keep_mutant(rec, dl, mutation=None):
    """the all-pairs rule over one list in plain loops, with one clause changed (None: the rule itself)"""
    rec = np.asarray(rec, np.int32)
    rec = rec.reshape(len(rec), rec.shape[-1] if len(rec) else 12)
    s = np.ascontiguousarray(rec[:, 5]).view(np.float32)

    def cov(a, b):
        xa, ya, wa, ha = (int(v) for v in a)
        xb, yb, wb, hb = (int(v) for v in b)
        cx, cy = 2 * xb + wb, 2 * yb + hb
        if mutation == "closed_interval":
            return wa > 0 and ha > 0 and 2 * xa <= cx <= 2 * (xa + wa) and 2 * ya <= cy <= 2 * (ya + ha)
        return wa > 0 and ha > 0 and 2 * xa <= cx < 2 * (xa + wa) and 2 * ya <= cy < 2 * (ya + ha)

    keep = ~np.isnan(s)
    for i in range(len(rec)):
        for j in range(len(rec)):
            if i == j or np.isnan(s[i]) or np.isnan(s[j]) or rec[i, 0] != rec[j, 0]:
                continue
            d = abs(int(rec[i, 2]) - int(rec[j, 2]))
            if (d >= dl) if mutation == "level_less_than_dl" else (d > dl):
                continue
            if mutation == "own_plane_excluded" and rec[i, 2] == rec[j, 2] and rec[i, 1] == rec[j, 1]:
                continue
            a, b = rec[i, 8:12], rec[j, 8:12]
            if not (cov(a, b) if mutation == "one_direction" else cov(a, b) or cov(b, a)):
                continue
            if mutation == "greater_equal":
                jb = s[j] >= s[i]
            elif mutation == "tie_to_later":
                jb = s[j] > s[i] or (s[j] == s[i] and j > i)
            else:
                jb = s[j] > s[i] or (s[j] == s[i] and j < i)
            if jb:
                keep[i] = False
    return keep


# ---- built pyramids ------------------------------------------------------------------------------------------------------------
def stepped_plane(rng, rows, cols, dtype, levels=5):
    return (np.round(rng.standard_normal((rows, cols)) * levels) / 4.0).astype(dtype)


def built_frame(seed, dtype, sizes, scales, root_ksize, pad=(0, 0), nan_rate=0.02):
    """a pyramid of random stepped planes: sizes[l] = (rows, cols) before the pad, scales[l], root types drawn per cell"""
    rng = np.random.default_rng(seed)
    out = []
    for (r, c), s in zip(sizes, scales):
        if r * c == 0:
            out.append(S.Level(float(s), [np.zeros((0, 0), dtype) for _ in root_ksize], [np.zeros((0, 0), np.int32) for _ in root_ksize]))
            continue
        R, Cc = r + 2 * pad[1], c + 2 * pad[0]
        rv, ri = [], []
        for ks in root_ksize:
            v = stepped_plane(rng, R, Cc, dtype)
            v[rng.random((R, Cc)) < nan_rate] = np.nan
            rv.append(v)
            ri.append(rng.integers(0, len(ks), (R, Cc)).astype(np.int32))
        out.append(S.Level(float(s), rv, ri, pad[0], pad[1]))
    return out


def plane_frames(dtype):
    """(name, levels, root_ksize, thresh): see the module's docstring"""
    geo = lambda n, s0, per: [np.float32(s0 * 2 ** (i / per)) for i in range(n)]
    sz = lambda n, r, c, per: [(max(int(r / 2 ** (i / per)), 0), max(int(c / 2 ** (i / per)), 0)) for i in range(n)]
    return [
        ("one_component", built_frame(1, dtype, sz(6, 14, 18, 3), geo(6, 4.0, 3), [[5]]), [[5]], -0.3),
        ("filter_sides_and_components", built_frame(2, dtype, sz(7, 13, 17, 3), geo(7, 4.0, 3), [[5, 3], [7], [4, 6, 2]]),
         [[5, 3], [7], [4, 6, 2]], 0.2),
        ("padded_2_2", built_frame(3, dtype, sz(6, 12, 15, 3), geo(6, 4.0, 3), [[5, 3], [6]], pad=(2, 2)), [[5, 3], [6]], -0.2),
        # a fine octave: three levels at half the bin size first, the scales still ascending; the last level is empty
        ("fine_octave_and_empty_level", built_frame(4, dtype, sz(3, 24, 30, 3) + sz(6, 12, 15, 3) + [(0, 0)],
                                                    geo(3, 2.0, 3) + geo(6, 4.0, 3) + [np.float32(20.0)], [[5], [3, 5]]),
         [[5], [3, 5]], 0.0),
        ("every_cell_eligible", built_frame(5, dtype, sz(5, 9, 11, 2), geo(5, 4.0, 2), [[5, 4]], nan_rate=0.0), [[5, 4]], -1e30),
    ]


# ---- the CPU oracle's root planes of a frame -------------------------------------------------------------------------------------
def root_ksizes(model):
    flat = model.flatten()
    return [[int(flat.filter_ksize[f]) for f in model.filterid[c][0]] for c in range(flat.ncomponents)]


def frame_levels(oracle, flat, im, dtype):
    """the frame's levels (scalenms.Level, no masks) from the CPU oracle"""
    feats, sc = oracle.features_pyramid(flat, im, dtype)
    out = []
    for f, s in zip(feats, sc):
        if f.size == 0:
            out.append(S.Level(float(s), [np.zeros((0, 0), dtype)] * flat.ncomponents, [np.zeros((0, 0), np.int32)] * flat.ncomponents))
            continue
        resp = oracle.responses(flat, f)
        res = [oracle.dp_min(flat, c, resp) for c in range(flat.ncomponents)]
        out.append(S.Level(float(s), [r[3] for r in res], [r[4] for r in res]))
    return out


def eligible_planes(levels, thresh):
    """uint8 planes [l][c]: rootv > thresh in the planes' dtype, and the level's mask where it has one"""
    out = []
    for L in levels:
        row = []
        for c, v in enumerate(L.rootv):
            e = np.asarray(v) > np.asarray(v).dtype.type(thresh)
            if L.mask is not None and L.mask[c] is not None:
                e = e & (np.asarray(L.mask[c]) != 0)
            row.append(e.astype(np.uint8))
        out.append(row)
    return out


def with_root_nms(levels, thresh, sz):
    """the levels with gridnms.grid_nms_ref's bytes (eligibility rootv > thresh) as their masks"""
    from partsbaseddetector_amd import gridnms
    out = []
    for L in levels:
        masks = [gridnms.grid_nms_ref(v, sz, np.asarray(v) > np.asarray(v).dtype.type(thresh)) if np.asarray(v).size else None
                 for v in L.rootv]
        out.append(S.Level(L.scale, L.rootv, L.rooti, L.padx, L.pady, masks))
    return out


def constant_frame():
    return np.full((48, 64, 3), 128, np.uint8)


def tied_neighbour_pairs(rec, dl):
    """(ordered pairs of neighbouring records with equal float scores, those on different levels)"""
    rec = np.asarray(rec, np.int32)
    s = np.ascontiguousarray(rec[:, 5]).view(np.float32)
    total = cross = 0
    for i in range(len(rec)):
        for j in np.flatnonzero((s == s[i]) & (np.abs(rec[:, 2] - rec[i, 2]) <= dl)):
            if j != i and S.neighbours(rec[i, 8:12], rec[i, 2], rec[j, 8:12], rec[j, 2], dl):
                total += 1
                cross += int(rec[i, 2] != rec[j, 2])
    return total, cross
