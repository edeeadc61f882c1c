"""Built planes for the grid NMS (pbd_grid_nms, gridnms.grid_nms_ref; include/pbd.h states the contract).

Every case is a plane of float64 values (cast by the tests to the type under test), a window size, an optional mask, the
properties it promises to reach (`reach`, checked by test_grid_nms_cpu.py against the events of a literal restatement of
src/nms.cpp) and, for the small ones, the hand-worked list of maxima (`want`, as (y, x) pairs; `want32` where float32 differs).

Events a plane can reach:
  clipped_block        a block cut short by the plane's edge
  clipped_window       a window cut short by the plane's edge
  empty_block          a block without an eligible element
  empty_neighbourhood  a candidate whose neighbourhood holds no eligible element
  tie_in_block         a block whose largest value occurs more than once
  tie_across           a candidate equal to its neighbourhood's largest value (dropped)
  diagonal_only        a candidate beaten only by cells of a diagonally adjacent block
  masked_larger        a kept candidate with a larger, ineligible neighbour
  beaten               a candidate smaller than a neighbour
  kept                 a maximum
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

SIZES = (0, 1, 2, 3, 4, 6, 7, 8, 15, 16, 31, 63, 100)     # 6 | 7: the two sides of the kernel variants' switch
FLT_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(1e-45))


@dataclass
class Case:
    name: str
    src: np.ndarray
    sz: int
    mask: Optional[np.ndarray] = None
    reach: Tuple[str, ...] = ()
    want: Optional[List[Tuple[int, int]]] = None
    want32: Optional[List[Tuple[int, int]]] = None      # float32 answer when it differs from float64's
    big: bool = False                                    # left out of the exhaustive CPU mutation runs

    def plane(self, dtype):
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(self.src.astype(dtype))

    def answer(self, dtype):
        return self.want32 if (np.dtype(dtype) == np.float32 and self.want32 is not None) else self.want


def _a(rows):
    return np.array(rows, np.float64)


def quantised(seed, rows, cols, levels):
    """a smooth random plane rounded to `levels` values: many exact ties, inside blocks and across them"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    z = sum(np.sin(y / a + p) * np.cos(x / b + q) for a, b, p, q in rng.uniform(2, 15, (4, 4)))
    return np.round((z - z.min()) / (z.max() - z.min()) * (levels - 1)).astype(np.float64) - 1.0


def smooth(seed, rows, cols):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    return sum(np.sin(y / a + p) * np.cos(x / b + q) for a, b, p, q in rng.uniform(1.5, 9, (5, 4))) + 1e-3 * rng.standard_normal((rows, cols))


def cases() -> List[Case]:
    out: List[Case] = []
    add = out.append
    # ---- plane shapes
    add(Case("one_by_one", _a([[5]]), 1, reach=("clipped_block", "empty_neighbourhood", "kept"), want=[(0, 0)]))
    row = _a([[1, 3, 2, 5, 4, 5, 0]])
    add(Case("one_row", row, 1, reach=("clipped_block", "clipped_window", "beaten", "kept"), want=[(0, 1), (0, 3), (0, 5)]))
    add(Case("one_column", row.T.copy(), 1, reach=("clipped_block", "clipped_window", "beaten", "kept"), want=[(1, 0), (3, 0), (5, 0)]))
    add(Case("smaller_than_a_block", np.arange(6, dtype=np.float64).reshape(2, 3), 5,
             reach=("clipped_block", "clipped_window", "empty_neighbourhood"), want=[(1, 2)]))
    add(Case("multiple_of_block", smooth(1, 9, 12), 2, reach=("kept", "beaten")))
    add(Case("not_a_multiple", smooth(2, 10, 13), 2, reach=("clipped_block", "kept", "beaten")))
    add(Case("empty_0xN", np.zeros((0, 5)), 2, want=[]))
    add(Case("empty_Mx0", np.zeros((4, 0)), 1, want=[]))
    # ---- ties
    add(Case("tie_inside_block_first_kept", _a([[7, 7], [7, 1]]), 1, reach=("tie_in_block", "empty_neighbourhood"), want=[(0, 0)]))
    z = np.zeros((3, 6)); z[0, 2] = 9; z[2, 4] = 9
    add(Case("tie_adjacent_blocks_distance_sz", z, 2, reach=("tie_across",), want=[]))
    z = np.zeros((3, 6)); z[0, 2] = 9; z[0, 5] = 9
    add(Case("tie_distance_sz_plus_1", z, 2, reach=("kept",), want=[(0, 2), (0, 5)]))
    # ---- neighbourhood geometry
    z = np.zeros((4, 4)); z[1, 1] = 5; z[2, 2] = 6
    add(Case("beaten_from_diagonal_block_only", z, 1, reach=("diagonal_only", "beaten", "kept"), want=[(2, 2)]))
    z = -np.ones((5, 5)); z[0, 3] = 4; z[4, 0] = 3
    # (0, 0) as well: its clipped window is its own block, so nothing is left to beat it
    add(Case("window_clipped_by_edge", z, 1, reach=("clipped_window", "clipped_block", "kept"), want=[(0, 0), (0, 3), (4, 0)]))
    # ---- block versus window
    add(Case("window_max_not_block_candidate", _a([[7, 1], [1, 7]]), 1, reach=("tie_in_block",), want=[(0, 0)]))
    add(Case("beaten_by_a_beaten_neighbour", _a([[1, 0, 5, 0, 6, 0, 7, 0, 0]]), 2, reach=("beaten", "kept"), want=[(0, 6)]))
    # ---- degenerate planes
    add(Case("constant_one_block", np.full((3, 3), 2.5), 2, reach=("tie_in_block", "empty_neighbourhood"), want=[(0, 0)]))
    # the first block's candidate is (0, 0), whose clipped window is its own block: kept; the second block's ties with the first
    add(Case("constant_two_blocks", np.full((3, 6), 2.5), 2, reach=("tie_in_block", "tie_across", "empty_neighbourhood"), want=[(0, 0)]))
    add(Case("ramp", np.arange(20, dtype=np.float64).reshape(4, 5), 2, reach=("clipped_block", "beaten", "kept"), want=[(3, 4)]))
    add(Case("lone_negative_maximum", _a([[-3]]), 4, reach=("empty_neighbourhood",), want=[(0, 0)]))
    # ---- special values
    nan, inf = np.nan, np.inf
    sp = _a([[nan, nan, 0.0, -0.0, inf, 1.0],
             [nan, nan, -0.0, DENORM, 2.0, inf],
             [-inf, -inf, FLT_MAX, 1.0, -DENORM, 0.0],
             [-inf, nan, 1.0, FLT_MAX, 0.0, -0.0]])
    add(Case("special_values_sz1", sp, 1, reach=("empty_block", "tie_in_block", "kept")))
    add(Case("special_values_sz2", sp, 2, reach=("tie_in_block", "clipped_block")))
    add(Case("signed_zeros_tie", _a([[-1, -0.0, 0.0, -1]]), 1, reach=("tie_across",), want=[]))
    add(Case("signed_zeros_first_kept", _a([[-0.0, 0.0]]), 1, reach=("tie_in_block",), want=[(0, 0)]))
    add(Case("inf_ties_inf", _a([[0, inf, inf, 0]]), 1, reach=("tie_across",), want=[]))
    add(Case("all_nan", np.full((3, 5), nan), 1, reach=("empty_block",), want=[]))
    add(Case("nan_neighbours_only", _a([[nan, 1.0, nan, nan]]), 1, reach=("empty_block", "empty_neighbourhood"), want=[(0, 1)]))
    e = 2.0 ** -40
    add(Case("f64_difference_below_float", _a([[0, 1 + e, 1, 0]]), 1, reach=("kept",), want=[(0, 1)], want32=[]))
    # ---- masks
    add(Case("mask_hides_larger_neighbour", _a([[0, 5, 9, 0]]), 1, mask=np.array([[1, 1, 0, 1]], np.uint8),
             reach=("masked_larger", "empty_neighbourhood"), want=[(0, 1), (0, 3)]))
    m = np.full((4, 6), 255, np.uint8); m[0:2, 2:4] = 0
    add(Case("fully_masked_block", smooth(3, 4, 6), 1, mask=m, reach=("empty_block", "kept")))
    add(Case("all_zero_mask", smooth(4, 5, 7), 2, mask=np.zeros((5, 7), np.uint8), reach=("empty_block",), want=[]))
    rng = np.random.default_rng(9)
    add(Case("random_mask", smooth(5, 23, 31), 2, mask=(rng.random((23, 31)) < 0.6).astype(np.uint8) * 3,
             reach=("masked_larger", "beaten", "kept")))
    # ---- every window size, on a plane with ties and one with NaN holes
    q = quantised(6, 37, 53, 9)
    holes = smooth(7, 37, 53)
    holes[rng.random((37, 53)) < 0.1] = nan
    for sz in SIZES:
        add(Case(f"quantised_sz{sz}", q, sz, reach=("kept",) if sz else ()))
        add(Case(f"holes_sz{sz}", holes, sz, reach=("kept",)))
    # ---- larger inputs
    big = quantised(8, 268, 478, 4)
    add(Case("big_quantised_sz2", big, 2, reach=("tie_in_block", "tie_across", "clipped_block"), big=True))
    add(Case("big_quantised_sz7", big, 7, reach=("tie_in_block", "tie_across", "clipped_block"), big=True))
    return out


def many_planes(n=3000, seed=12):
    """n small planes of assorted sizes (some empty) for one call: more (plane, block) pairs than a capped grid has waves"""
    rng = np.random.default_rng(seed)
    shapes = [(int(r), int(c)) for r, c in zip(rng.integers(0, 8, n), rng.integers(0, 9, n))]
    return [np.round(rng.standard_normal(s) * 2) for s in shapes]


# ---- the detect path's inputs (test_gpu_root_nms.py; their conditions are checked on the CPU oracle in test_grid_nms_cpu.py)
ROOT_NMS_SIZES = (1, 2, 5)
ROOT_NMS_THRESH = 0.6


def root_nms_frames():
    from partsbaseddetector_amd import synth
    return [synth.synthetic_frame(31 + i, 120, 150, 3) for i in range(4)]
