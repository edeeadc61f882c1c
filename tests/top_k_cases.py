"""Built segments and record lists for the top-K selection (pbd_top_k_cells, pbd_top_k, topk.py; include/pbd.h states the rule).

Every case is a list of segments of float64 values (cast by the tests to the type under test; `segs32` where float32 needs values
of its own), one K for the call, optional masks, the events it promises to reach (`reach`, checked by test_top_k_cpu.py) and, for
the small ones, the hand-worked kept indices of every segment (`want`; `want32` where float32 differs).

Events a case can reach (in some segment):
  empty_segment     a segment of length 0
  multi_tile        a segment longer than one tile of the kernel (1024 elements)
  longer_than_grid  more segments than a capped grid has workgroups or waves
  k_zero            K = 0
  k_below           0 < K < eligible
  k_at              K = eligible > 0
  k_above           K > eligible
  cut_in_tie        the K-th best value also occurs among the dropped elements
  two_each_side     ... with at least two kept and two dropped elements of that value
  tie_across_tiles  ... whose kept elements of that value lie in more than one tile
  all_equal         every eligible element has one value (at least two of them)
  low_byte_only     the eligible elements' keys differ only in their lowest byte
  sign_only         a kept element whose negation is a dropped eligible element
  zeros_cut         the cut falls between a -0.0 and a +0.0
  inf_tie           +Inf twice, one kept and one dropped
  nan_hole          a NaN element
  mask_hides_best   the largest value that is not NaN is masked out
  mask_all_zero     a mask without a non-zero byte over a segment with elements
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

TILE = 1024
LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025)
LONG = 70000
FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(1e-45))
EVENTS = ("empty_segment", "multi_tile", "longer_than_grid", "k_zero", "k_below", "k_at", "k_above", "cut_in_tie", "two_each_side",
          "tie_across_tiles", "all_equal", "low_byte_only", "sign_only", "zeros_cut", "inf_tie", "nan_hole", "mask_hides_best",
          "mask_all_zero")


@dataclass
class Case:
    name: str
    segs: List[np.ndarray]
    k: int
    masks: Optional[List[Optional[np.ndarray]]] = None
    reach: Tuple[str, ...] = ()
    want: Optional[List[List[int]]] = None
    want32: Optional[List[List[int]]] = None             # float32 answer when it differs from float64's
    segs32: Optional[List[np.ndarray]] = None            # float32 values when they are not the float64 ones, cast
    big: bool = False                                    # left out of the literal restatement and the mutation runs

    def values(self, dtype):
        src = self.segs32 if (np.dtype(dtype) == np.float32 and self.segs32 is not None) else self.segs
        with np.errstate(over="ignore"):
            return [np.ascontiguousarray(np.asarray(s).astype(dtype)) for s in src]

    def mask_list(self):
        """a uint8 array per segment (all ones where the case has none), or None"""
        if self.masks is None:
            return None
        return [np.ones(len(s), np.uint8) if m is None else np.asarray(m, np.uint8) for s, m in zip(self.segs, self.masks)]

    def answer(self, dtype):
        return self.want32 if (np.dtype(dtype) == np.float32 and self.want32 is not None) else self.want


def _a(v):
    return np.array(v, np.float64)


def stepped(seed, n, levels):
    """n random values rounded to about `levels` distinct ones: many exact ties"""
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal(n) * levels / 6.0) / 4.0


def low_byte(dtype, seed=3):
    """256 values of `dtype` whose bit patterns differ only in the lowest byte, shuffled, some twice"""
    rng = np.random.default_rng(seed)
    low = np.concatenate([rng.permutation(256), rng.integers(0, 256, 44)])
    if np.dtype(dtype) == np.float32:
        return (np.uint32(0x40490F00) | low.astype(np.uint32)).view(np.float32)
    return (np.uint64(0x400921FB54442D00) | low.astype(np.uint64)).view(np.float64)


SPECIAL = _a([np.nan, -0.0, 0.0, DENORM, -DENORM, FLT_MAX, np.inf, np.inf, -np.inf, np.nan, 0.0, -FLT_MAX])
SPECIAL_ORDER = [6, 7, 5, 3, 1, 2, 10, 4, 11, 8]        # best first, worked by hand: the two NaN never appear


def cases() -> List[Case]:
    out: List[Case] = []
    add = out.append
    # ---- segment lengths around the wave, the tile and far beyond, K on every side of the eligible count
    segs = [stepped(10 + i, n, 40) for i, n in enumerate(LENGTHS)]
    add(Case("lengths_k0", segs, 0, reach=("k_zero", "empty_segment")))
    add(Case("lengths_k1", segs, 1, reach=("k_above", "k_at", "k_below", "empty_segment", "multi_tile")))
    add(Case("lengths_k64", segs, 64, reach=("k_above", "k_at", "k_below", "cut_in_tie", "multi_tile")))
    add(Case("lengths_k1000", segs, 1000, reach=("k_above", "k_below", "cut_in_tie")))
    add(Case("lengths_k1024", segs, 1024, reach=("k_at", "k_below")))
    add(Case("long_between_short", [stepped(20, 37, 9), stepped(21, LONG, 60), stepped(22, 5, 3)], 12345,
             reach=("multi_tile", "k_above", "k_below", "cut_in_tie", "two_each_side", "tie_across_tiles"), big=True))
    rng = np.random.default_rng(23)
    add(Case("tiny_3000", [np.round(rng.standard_normal(int(n)) * 2) for n in rng.integers(0, 8, 3000)], 2,
             reach=("longer_than_grid", "empty_segment", "k_above", "k_at", "k_below", "cut_in_tie"), big=True))
    add(Case("medium_5000", [stepped(3000 + i, int(n), 12) for i, n in enumerate(rng.integers(900, 1200, 5000))], 300,
             reach=("longer_than_grid", "multi_tile", "k_below", "cut_in_tie", "two_each_side"), big=True))
    # ---- ties
    add(Case("cut_inside_a_run", [_a([5, 3, 3, 3, 3, 1])], 3, reach=("cut_in_tie", "two_each_side", "k_below"), want=[[0, 1, 2]]))
    add(Case("cut_inside_a_scattered_run", [_a([3, 9, 3, 1, 3, 8, 3, 3])], 4, reach=("two_each_side",), want=[[0, 1, 2, 5]]))
    add(Case("cut_after_a_run", [_a([5, 3, 3, 1])], 3, reach=("k_below",), want=[[0, 1, 2]]))
    add(Case("all_equal", [np.full(100, 2.5)], 7, reach=("all_equal", "two_each_side"), want=[list(range(7))]))
    add(Case("all_equal_negative_long", [np.full(3000, -1.0)], 1500, reach=("all_equal", "tie_across_tiles", "multi_tile"),
             want=[list(range(1500))]))
    z = np.ones(2500); z[[7, 1030, 2499]] = 2.0
    add(Case("run_over_three_tiles", [z], 2100, reach=("tie_across_tiles", "two_each_side"),
             want=[sorted([7, 1030, 2499] + [i for i in range(2500) if i not in (7, 1030, 2499)][:2097])]))
    add(Case("two_segments_cut_alike", [_a([1, 2, 2, 2]), _a([2, 2, 2, 1])], 2, reach=("cut_in_tie",), want=[[1, 2], [0, 1]]))
    # ---- keys
    add(Case("low_byte_only", [low_byte(np.float64)], 100, segs32=[low_byte(np.float32)], reach=("low_byte_only", "cut_in_tie")))
    add(Case("low_byte_only_negative", [-low_byte(np.float64)], 17, segs32=[-low_byte(np.float32)], reach=("low_byte_only",)))
    add(Case("sign_only", [_a([1.5, -1.5, 2.0, -2.0])], 2, reach=("sign_only",), want=[[0, 2]]))
    add(Case("sign_only_one_pair", [_a([-7.0, 7.0])], 1, reach=("sign_only",), want=[[1]]))
    add(Case("negatives", [_a([-3, -1, -2, -1, -5])], 2, reach=("k_below",), want=[[1, 3]]))
    add(Case("negatives_cut_in_tie", [_a([-3, -1, -2, -1, -2, -2])], 3, reach=("cut_in_tie",), want=[[1, 2, 3]]))
    for k in range(1, 12):
        reach = ["nan_hole"]
        reach += {1: ["inf_tie", "cut_in_tie"], 5: ["zeros_cut", "cut_in_tie"], 10: ["k_at"], 11: ["k_above"]}.get(k, [])
        add(Case(f"special_k{k}", [SPECIAL], k, reach=tuple(reach), want=[sorted(SPECIAL_ORDER[:k])]))
    add(Case("zeros_first_wins", [_a([-1, -0.0, 0.0, -0.0, -1])], 2, reach=("zeros_cut",), want=[[1, 2]]))
    add(Case("denormals", [_a([DENORM, 2 * DENORM, -DENORM, 0.0, 3 * DENORM])], 3, reach=("k_below",), want=[[0, 1, 4]]))
    add(Case("all_nan", [np.full(9, np.nan)], 3, reach=("nan_hole", "k_above"), want=[[]]))
    e = 2.0 ** -40
    add(Case("f64_difference_below_float", [_a([1, 1 + e, 0])], 1, want=[[1]], want32=[[0]]))
    # ---- masks
    add(Case("mask_hides_the_best", [_a([1, 9, 5, 3])], 2, masks=[np.array([1, 0, 1, 1], np.uint8)], reach=("mask_hides_best",),
             want=[[2, 3]]))
    add(Case("mask_bytes_other_than_255", [_a([4, 3, 2, 1])], 2, masks=[np.array([0, 7, 0, 128], np.uint8)], reach=("k_at",),
             want=[[1, 3]]))
    add(Case("all_zero_mask", [stepped(30, 50, 9), _a([1, 2])], 3, masks=[np.zeros(50, np.uint8), None],
             reach=("mask_all_zero", "k_above"), want=[[], [0, 1]]))
    holes = stepped(31, 5000, 80)
    holes[rng.random(5000) < 0.1] = np.nan
    add(Case("holes_and_random_mask", [holes, stepped(32, 700, 5)], 777,
             masks=[(rng.random(5000) < 0.6).astype(np.uint8) * 3, (rng.random(700) < 0.5).astype(np.uint8)],
             reach=("nan_hole", "k_below", "k_above", "cut_in_tie", "multi_tile")))
    return out


def many_segments(n=20000, seed=12):
    """n short segments (some empty) for one device-form call: more segments than a capped grid has waves"""
    rng = np.random.default_rng(seed)
    return [np.round(rng.standard_normal(int(m)) * 2) for m in rng.integers(0, 6, n)]


# ---- record lists (pbd_top_k*): per case the scores of every frame index, K, and the events of the list above it reaches
RECORD_CASES = (
    ("cut_inside_a_run", {0: [5, 3, 3, 3, 3, 1]}, 3, ("cut_in_tie", "two_each_side")),
    ("frames_without_records", {0: [1, 2], 2: [4, 4, 4], 5: [7]}, 2, ("k_at", "k_above", "k_below", "cut_in_tie")),
    ("k_zero", {0: [1, 2], 1: [3]}, 0, ("k_zero",)),
    ("nan_score", {0: [np.nan, 1, np.nan, 2], 1: [np.nan]}, 3, ("nan_hole", "k_above")),
    ("special", {1: list(SPECIAL)}, 5, ("zeros_cut", "nan_hole")),
    ("all_equal", {0: [2.5] * 100, 1: [2.5] * 3}, 7, ("all_equal", "k_above")),
    ("sign_only", {3: [1.5, -1.5, 2.0, -2.0]}, 2, ("sign_only",)),
)
RECORD_COUNTS = (0, 1, 63, 64, 65, 5000)


def record_list(stride, scores_by_frame, frame_offset=0):
    """the records (n, stride) int32 of the frames' scores, grouped by ascending frame: nparts 1, every other word distinct"""
    rows = []
    for f in sorted(scores_by_frame):
        for s in scores_by_frame[f]:
            r = np.arange(stride, dtype=np.int32) + 1000 * (len(rows) + 1)
            r[0] = f + frame_offset
            r[1] = 0
            r[5] = np.array([s], np.float32).view(np.int32)[0]
            r[6] = 1
            rows.append(r)
    return np.array(rows, np.int32).reshape(len(rows), stride)


def random_records(stride, n, nframes, seed):
    """n records over nframes frames with stepped scores (ties) and a few NaN"""
    rng = np.random.default_rng(seed)
    frames = np.sort(rng.integers(0, nframes, n))
    scores = stepped(seed + 1, n, 20)
    scores[rng.random(n) < 0.05] = np.nan
    by = {}
    for f, s in zip(frames, scores):
        by.setdefault(int(f), []).append(s)
    return record_list(stride, by)


# ---- the detect path's inputs (test_gpu_top_k.py; their conditions are checked on the CPU oracle in test_top_k_cpu.py)
TOP_K_SWEEP = (1, 2, 5, 64, 65, 5000)
TOP_K_THRESH = 0.6
MIXED_SHAPES = ((120, 150), (100, 130), (140, 110))


def top_k_frames():
    """four 120 x 150 frames: two plain ones, one tiled 2 x 2 from its top-left quarter (its second and third best roots are equal), one
    constant grey (long runs of equal root scores once the threshold is lowered)"""
    from partsbaseddetector_amd import synth
    a = synth.synthetic_frame(31, 120, 150, 3)
    return [a, np.ascontiguousarray(np.tile(a[:60, :75], (2, 2, 1))), synth.synthetic_frame(32, 120, 150, 3),
            np.full((120, 150, 3), 128, np.uint8)]


def oracle_frame_values(oracle, flat, im):
    """one frame's rootv from the CPU oracle in the find's order: (level, component, y, x)"""
    feats, _ = oracle.features_pyramid(flat, im)
    out = []
    for f in feats:
        if f.size == 0:
            continue
        resp = oracle.responses(flat, f)
        for c in range(flat.ncomponents):
            out.append(np.asarray(oracle.dp_min(flat, c, resp)[3]).ravel())
    return np.concatenate(out)
