"""Hand-built candidate records for the model-testing calls (pbd_part_nms, pbd_best_overlap, pbd_eval_pck, pbd_eval_apk), shared
by tests/test_eval_cpu.py (the numpy yardstick against a literal restatement of the .m files) and tests/test_gpu_eval.py (the
device against the yardstick).  No detection is needed: a record is (frame, score, part boxes).

Each small case names the rule it is there for; test_eval_cpu.py asserts that changing that rule changes the case's result.
"""
import numpy as np

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import synth

OV03 = float(np.float32(0.3))


def model1():
    return M.synthetic_model(seed=1, pa=[0], nmix=1, interval=2, name="eval_1part")


def model2():
    return M.synthetic_model(seed=2, pa=[0, 1], nmix=1, interval=2, name="eval_2parts")


def model26():
    return M.synthetic_person_model()


def records(nparts, rows):
    """rows of (frame, score, [(x, y, w, h)] * nparts) -> (n, 8 + 4 nparts) int32 records"""
    rec = np.zeros((len(rows), 8 + 4 * nparts), np.int32)
    for i, (frame, score, boxes) in enumerate(rows):
        assert len(boxes) == nparts
        rec[i, 0] = frame
        rec[i, 5] = np.float32(score).view(np.int32)
        rec[i, 6] = nparts
        rec[i, 8:] = np.asarray(boxes, np.int64).astype(np.int32).ravel()
    return rec


def same(nparts, x, y, w, h):
    """every part the same box: the hull is that box too"""
    return [(x, y, w, h)] * nparts


def spread(nparts, first, rest):
    return [first] + [rest] * (nparts - 1)


# ---- part NMS: one frame each, (name, overlap, max_boxes, rows, kept indices in pick order) --------------------------------
def nms_cases(nparts):
    """the kept indices are worked out by hand from the rules of include/pbd.h"""
    sq = lambda x, y=0: same(nparts, x, y, 9, 9)          # a 10 x 10 box (inclusive area 100)
    cases = [
        # o == overlap exactly: 50 / 100 and 25 / 100 are not > overlap (>= would remove the second record)
        ("o_equals_half", 0.5, 1000, [(0, 2.0, sq(0)), (0, 1.0, sq(5))], [0, 1]),
        ("o_equals_quarter", 0.25, 1000, [(0, 2.0, sq(0)), (0, 1.0, sq(5, 5))], [0, 1]),
        # (w * h) / area > 0.3f is false here, w * h > 0.3f * area is true (found by search: test_eval_cpu.py repeats the check)
        ("division_not_product", OV03, 1000, [(0, 2.0, same(nparts, 0, 0, 1634738417, 1941643311)),
                                              (0, 1.0, same(nparts, 0, 0, 764851962, 1244977797))], [0, 1]),
        # the divisor is the PICKER's area: a large pick leaves the small record inside it, a small pick removes the large one
        ("large_then_small", OV03, 1000, [(0, 2.0, same(nparts, 0, 0, 99, 99)), (0, 1.0, sq(10, 10))], [0, 1]),
        ("small_then_large", OV03, 1000, [(0, 1.0, same(nparts, 0, 0, 99, 99)), (0, 2.0, sq(10, 10))], [1]),
        # A removes B, B would remove C, A does not: C survives because B left before its turn
        ("chain", OV03, 1000, [(0, 3.0, sq(0)), (0, 2.0, sq(4)), (0, 1.0, sq(8))], [0, 2]),
        # equal scores: the LAST in the list is picked first (and here removes the first)
        ("tie_overlapping", OV03, 1000, [(0, 1.0, sq(0)), (0, 1.0, sq(1))], [1]),
        ("tie_apart", OV03, 1000, [(0, 1.0, sq(0)), (0, 1.0, sq(50)), (0, 2.0, sq(100))], [2, 1, 0]),
        # -0.0 and +0.0 tie: the last is picked (a bit-pattern order would pick +0.0)
        ("signed_zeros", OV03, 1000, [(0, 0.0, sq(0)), (0, -0.0, sq(1))], [1]),
        # overlap >= 1: the pick itself still leaves (Matlab would loop forever)
        ("overlap_one", 1.0, 1000, [(0, 2.0, sq(0)), (0, 1.0, sq(0))], [0, 1]),
        # the cut: equal scores straddle it, the first in list order stay; survivors come out in pick order
        ("cut_ties", OV03, 5, [(0, s, sq(20 * i)) for i, s in enumerate([3.0, 5.0, 3.0, 1.0, 3.0, 4.0, 3.0, 2.0])], [1, 5, 4, 2, 0]),
        # a record that the cut drops cannot remove anything: at max_boxes 1 only the highest is left
        ("cut_to_one", OV03, 1, [(0, 1.0, sq(0)), (0, 3.0, sq(100)), (0, 2.0, sq(200))], [1]),
    ]
    if nparts >= 2:
        far_a, far_b = (1000, 0, 9, 9), (0, 1000, 9, 9)
        cases += [
            # part 0 coincides, every other part and the hulls are far apart: removed through one part box only
            ("one_part_only", OV03, 1000, [(0, 2.0, spread(nparts, (0, 0, 9, 9), far_a)), (0, 1.0, spread(nparts, (0, 0, 9, 9), far_b))],
             [0]),
            # no part meets its counterpart, the hulls coincide: removed through the hull only
            ("hull_only", OV03, 1000, [(0, 2.0, [(0, 0, 9, 9)] * (nparts - 1) + [(90, 90, 9, 9)]),
                                       (0, 1.0, [(90, 0, 9, 9)] * (nparts - 1) + [(0, 90, 9, 9)])], [0]),
        ]
    return cases


def random_records(seed, n, nparts, frame, span=600, ties=True, nan=0, negative=0):
    """n records of one frame: part boxes scattered around a random centre inside span x span, scores on a coarse grid (many
    ties, both zeros); `nan` records get a NaN score and `negative` a part of negative width"""
    if n == 0:
        return np.zeros((0, 8 + 4 * nparts), np.int32)
    cx = synth.randint(seed, n, 0, span, 1)
    cy = synth.randint(seed, n, 0, span, 2)
    off = synth.randint(seed, n * nparts * 2, -25, 25, 3).reshape(n, nparts, 2)
    size = synth.randint(seed, n * nparts * 2, 4, 40, 4).reshape(n, nparts, 2)
    sc = synth.normalish(seed, n, 5).astype(np.float32)
    if ties:
        sc = (np.round(sc * 16) / 16).astype(np.float32)
        sc[::7] = 0.0
        sc[3::14] = -0.0
    rec = np.zeros((n, 8 + 4 * nparts), np.int32)
    rec[:, 0] = frame
    rec[:, 1] = 0
    rec[:, 5] = sc.view(np.int32)
    rec[:, 6] = nparts
    parts = rec[:, 8:].reshape(n, nparts, 4)
    parts[:, :, 0] = cx[:, None] + off[:, :, 0]
    parts[:, :, 1] = cy[:, None] + off[:, :, 1]
    parts[:, :, 2:] = size
    for k in range(nan):
        rec[(k * 37 + 5) % n, 5] = np.float32(np.nan).view(np.int32)
    for k in range(negative):
        parts[(k * 53 + 11) % n, k % nparts, 2] = -7
    return rec


NMS_FRAME_COUNTS = [0, 1, 2, 64, 0, 65, 999, 1000, 1001, 1500]   # an empty frame first and in the middle


def nms_many_frames(nparts=2, frame_offset=0):
    """frames of NMS_FRAME_COUNTS records in one call"""
    parts = [random_records(100 + f, n, nparts, f + frame_offset, span=900, nan=2 if n >= 64 else 0, negative=1 if n >= 64 else 0)
             for f, n in enumerate(NMS_FRAME_COUNTS)]
    return np.concatenate(parts), len(NMS_FRAME_COUNTS)


# ---- best overlap ------------------------------------------------------------------------------------------------------------
def best_cases(nparts=2):
    """-> rows, gtbox (nframes, 4), overlap, the index chosen per frame (None: not found).  Frame 1 has no records, frame 2 a
    NaN ground-truth row"""
    gt = np.array([[0, 0, 9, 9], [0, 0, 9, 9], [0, np.nan, 9, 9], [0, 0, 99, 99], [0, 0, 9, 9], [0, 0, 99, 99]], np.float64)
    inside = lambda: spread(nparts, (-1, -1, 2, 2), (8, 8, 2, 2))       # centres (0, 0) and (9, 9): covers the 10 x 10 box
    half = lambda: spread(nparts, (-1, -1, 2, 2), (3, 8, 2, 2))        # centres (0, 0) and (4, 9): 5 x 10 of 100 = 0.5
    big = lambda: spread(nparts, (-1, -1, 2, 2), (98, 98, 2, 2))       # centres (0, 0) and (99, 99): covers the 100 x 100 box
    rows = [
        # frame 0, overlap 0.5: o == overlap does not pass; the tied best scores stand at both ends of the list
        (0, 9.0, half()), (0, 2.0, inside()), (0, 1.0, inside()), (0, 2.0, inside()),
        # frame 2: NaN ground truth, nothing found
        (2, 5.0, inside()),
        # frame 3: -0.0 and +0.0 tie, the first wins; the NaN score is never chosen
        (3, -0.0, big()), (3, float("nan"), big()), (3, 0.0, big()),
        # frame 4: only a failing record
        (4, 1.0, same(nparts, 500, 500, 4, 4)),
        # frame 5: a later, higher score
        (5, 1.0, big()), (5, 3.0, big()),
    ]
    return rows, gt, 0.5, [1, None, None, 5, None, 10]


# ---- PCK ---------------------------------------------------------------------------------------------------------------------
def pck_case(nparts=2):
    """four frames: a 3-4-5 triangle with dist == thresh * scale (a miss: strict), a hit, a frame that is not found, a NaN
    ground-truth point.  -> rows, found, gt_points, scale, thresh, pck"""
    at = lambda cx, cy: same(nparts, cx - 1, cy - 1, 2, 2)            # every part centred at (cx, cy)
    rows = [(0, 1.0, at(3, 4)), (1, 1.0, at(3, 4)), (2, 1.0, at(3, 4)), (3, 1.0, at(3, 4))]
    gt = np.zeros((4, nparts, 2))
    scale = np.array([10.0, 10.5, 100.0, 100.0])
    gt[3, 0, 0] = np.nan
    found = np.array([1, 1, 0, 1], np.int32)
    pck = np.full(nparts, 0.5)
    pck[0] = 0.25
    return rows, found, gt, scale, 0.5, pck


# ---- APK ---------------------------------------------------------------------------------------------------------------------
def apk_case(nparts=2):
    """-> rows, gt_offset, gt_points, gt_scale, thresh, the true-positive flags of part 0 in rank order.  All parts of a record
    are centred on one point and all points of an instance coincide, so every part sees the same geometry."""
    at = lambda cx, cy: same(nparts, cx - 1, cy - 1, 2, 2)
    inst = []                                         # (frame, x, y, scale)
    inst += [(0, 0, 0, 10.0), (0, 20, 0, 10.0)]       # frame 0: two instances, a detection half way is equidistant
    #                                                   frame 1: no ground truth
    inst += [(2, np.nan, np.nan, 10.0)]               # frame 2: the only instance is NaN
    inst += [(3, 0, 0, 10.0)]                         # frame 3: one instance, detected twice; distmin == thresh
    rows = [
        (0, 9.0, at(10, 0)),     # equidistant (d = 1.0 > 0.5): a false positive whichever instance is nearest
        (3, 8.0, at(3, 4)),      # dist 5 / scale 10 == thresh: a true positive (<=)
        (1, 8.0, at(0, 0)),      # no ground truth in the frame (ties the record above: list order decides the rank)
        (3, 7.0, at(0, 0)),      # the same instance again: a false positive
        (2, 6.0, at(0, 0)),      # all distances NaN: a false positive
        (0, 5.0, at(10, 3)),     # equidistant again, d = sqrt(109) / 10 > 0.5: false
    ]
    return _apk_pack(nparts, rows, inst, 4, 0.5) + ([0, 1, 0, 0, 0, 0],)


def apk_first_jmin_case(nparts=2):
    """the FIRST nearest instance is taken: the first record is equidistant from both instances of the frame and claims instance
    0, so the second record, near instance 0 only, is a false positive (with the last nearest it would be a true one)"""
    at = lambda cx, cy: same(nparts, cx - 1, cy - 1, 2, 2)
    inst = [(0, 0, 0, 100.0), (0, 20, 0, 100.0)]
    rows = [(0, 2.0, at(10, 0)), (0, 1.0, at(0, 0))]
    return _apk_pack(nparts, rows, inst, 1, 0.5) + ([1, 0],)


def apk_sum_order_case(nparts=2):
    """true positives at ranks 0, 1, 3 of 8 with 3 instances: ap = 0.9166666666666666 summed in ascending i, ...65 descending"""
    at = lambda cx, cy: same(nparts, cx - 1, cy - 1, 2, 2)
    inst = [(0, 0, 0, 10.0), (0, 100, 0, 10.0), (0, 200, 0, 10.0)]
    far = at(1000, 1000)
    rows = [(0, 8.0, at(0, 0)), (0, 7.0, at(100, 0)), (0, 6.0, far), (0, 5.0, at(200, 0)), (0, 4.0, far), (0, 3.0, far),
            (0, 2.0, far), (0, 1.0, far)]
    return _apk_pack(nparts, rows, inst, 1, 0.5) + ([1, 1, 0, 1, 0, 0, 0, 0],)


def _apk_pack(nparts, rows, inst, nframes, thresh):
    gt_offset = np.zeros(nframes + 1, np.int32)
    for f, _, _, _ in inst:
        gt_offset[f + 1:] += 1
    gt = np.zeros((len(inst), nparts, 2))
    for g, (_, x, y, _) in enumerate(inst):
        gt[g, :, 0] = x
        gt[g, :, 1] = y
    return rows, gt_offset, gt, np.array([s for _, _, _, s in inst], np.float64), thresh


def apk_random(seed, n, nparts, nframes=40, frame_offset=0):
    """n records over nframes frames with 0..3 instances each; scores with ties across frames"""
    rec = np.concatenate([random_records(seed + f, c, nparts, f + frame_offset, span=120)
                          for f, c in enumerate(np.bincount(synth.randint(seed, n, 0, nframes - 1, 9), minlength=nframes))])
    perm = np.argsort(synth.uniform_u32(seed, len(rec), 10), kind="stable")
    rec = rec[perm]                                   # any order
    counts = synth.randint(seed, nframes, 0, 3, 11)
    gt_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    G = int(gt_offset[-1])
    gt = synth.randint(seed, G * nparts * 2, 0, 120, 12).reshape(G, nparts, 2).astype(np.float64)
    gt[::5, 0, 0] = np.nan
    scale = 20.0 + synth.randint(seed, G, 0, 40, 13).astype(np.float64)
    return rec, gt_offset, gt, scale
