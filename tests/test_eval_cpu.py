"""The numpy yardstick of the model-testing calls (partsbaseddetector_amd/evaluation.py) against a second, literal restatement of
matlab/detection/nms.m, bestoverlap.m and matlab/evaluation/eval_pck.m, eval_apk.m, VOCap.m written here in 1-based coordinates
(no Octave is on the build machine), on the built cases of tests/eval_hard_cases.py; and those cases against what they promise.
For every rule of the contract, the restatement with that one rule changed differs from the yardstick on at least one case --
with one exception, stated in test_cut_order_cannot_be_seen.  Also: the C++ members compile, the library exports the new names.
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import eval_hard_cases as H
from partsbaseddetector_amd import evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the .m files, literally -------------------------------------------------------------------------------------------------
def box_matrix(rec, nparts):
    """detect.m's box matrix: [x1 y1 x2 y2] per part, then the score; 1-based (every formula depends on differences only)"""
    c = ev.corners(rec, nparts) + 1.0
    return np.concatenate([c.reshape(len(rec), 4 * nparts), ev.scores(rec).astype(np.float64)[:, None]], axis=1)


def m_sort(v, descend=False):
    """Matlab's stable sort (no NaN here): the 0-based index vector"""
    return sorted(range(len(v)), key=(lambda i: -v[i]) if descend else (lambda i: v[i]))


def m_nms(boxes, overlap, numpart, cut=1000, rule=None):
    """nms.m; `rule` changes one rule (None: the file as it is).  -> the picked row indices of the input"""
    rows = list(range(len(boxes)))
    if len(boxes) == 0:
        return []
    if len(boxes) > cut:
        I = m_sort(boxes[:, -1], descend=True)
        keep = I[:cut]
        if rule == "cut_keeps_list_order":
            keep = sorted(keep)
        rows = keep
        boxes = boxes[keep]
    n = len(boxes)
    x1 = np.zeros((n, numpart)); y1 = np.zeros((n, numpart)); x2 = np.zeros((n, numpart)); y2 = np.zeros((n, numpart))
    area = np.zeros((n, numpart))
    for p in range(numpart):
        x1[:, p] = boxes[:, 0 + p * 4]; y1[:, p] = boxes[:, 1 + p * 4]; x2[:, p] = boxes[:, 2 + p * 4]; y2[:, p] = boxes[:, 3 + p * 4]
        area[:, p] = (x2[:, p] - x1[:, p] + 1) * (y2[:, p] - y1[:, p] + 1)
    rx1 = x1.min(1); ry1 = y1.min(1); rx2 = x2.max(1); ry2 = y2.max(1)
    rarea = (rx2 - rx1 + 1) * (ry2 - ry1 + 1)
    x1 = np.c_[x1, rx1]; y1 = np.c_[y1, ry1]; x2 = np.c_[x2, rx2]; y2 = np.c_[y2, ry2]; area = np.c_[area, rarea]
    s = boxes[:, -1]
    I = m_sort(s)
    if rule == "tie_first":
        I = m_sort(s, descend=True)[::-1]      # among equal scores the FIRST of the list is picked first
    pick = []
    while len(I):
        i = I[-1]
        pick.append(i)
        J = np.array(I)
        xx1 = np.maximum(x1[i], x1[J]); yy1 = np.maximum(y1[i], y1[J]); xx2 = np.minimum(x2[i], x2[J]); yy2 = np.minimum(y2[i], y2[J])
        w = xx2 - xx1 + 1; w[w < 0] = 0
        h = yy2 - yy1 + 1; h[h < 0] = 0
        inter = w * h
        with np.errstate(all="ignore"):
            if rule == "other_area":
                o = inter / area[J]
            elif rule == "product":
                hit = (inter > overlap * area[i][None, :]).any(1)
            else:
                o = inter / area[i][None, :]
            if rule != "product":
                o = o.max(1)
                hit = o >= overlap if rule == "ge" else o > overlap
        hit[len(I) - 1] = True                 # project decision: the pick itself always leaves
        I = [j for j, gone in zip(I, hit) if not gone]
    return [rows[i] for i in pick]


def m_bestoverlap(boxes, gtbox, overlap, rule=None):
    """bestoverlap.m -> the chosen row or None"""
    if len(boxes) == 0 or gtbox is None:
        return None
    x1, y1, x2, y2 = gtbox
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    b = boxes[:, :(boxes.shape[1] // 4) * 4].reshape(len(boxes), -1, 4)
    bx = .5 * b[:, :, 0] + .5 * b[:, :, 2]
    by = .5 * b[:, :, 1] + .5 * b[:, :, 3]
    bx1 = bx.min(1); bx2 = bx.max(1); by1 = by.min(1); by2 = by.max(1)
    xx1 = np.maximum(x1, bx1); yy1 = np.maximum(y1, by1); xx2 = np.minimum(x2, bx2); yy2 = np.minimum(y2, by2)
    w = xx2 - xx1 + 1; w[w < 0] = 0
    h = yy2 - yy1 + 1; h[h < 0] = 0
    o = (w * h) / area
    I = np.flatnonzero(o >= overlap if rule == "ge" else o > overlap)
    if not len(I):
        return None
    sc = boxes[I, -1]
    ind = int(np.argmax(sc)) if rule != "tie_last" else len(sc) - 1 - int(np.argmax(sc[::-1]))
    return int(I[ind])


def m_eval_pck(ca, gt, scale_last, thresh, rule=None):
    """eval_pck.m with its threshold argument honoured: ca, gt (n, nparts, 2); the LAST frame's scale, as the file has it"""
    dist = np.zeros((ca.shape[1], len(ca)))
    for n in range(len(gt)):
        dist[:, n] = np.sqrt(((ca[n] - gt[n]) ** 2).sum(1))
    hit = dist <= thresh * scale_last if rule == "le" else dist < thresh * scale_last
    return hit.mean(1), dist


def m_vocap(rec, prec, rule=None):
    mrec = np.r_[0.0, rec, 1.0]
    mpre = np.r_[0.0, prec, 0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    idx = [i for i in range(1, len(mrec)) if mrec[i] != mrec[i - 1]]
    if rule == "descending_sum":
        idx = idx[::-1]
    ap = np.float64(0.0)
    for i in idx:
        ap = ap + (mrec[i] - mrec[i - 1]) * mpre[i]
    return float(ap)


def m_eval_apk(score, fr, point, gt_offset, gt_point, gt_scale, thresh, part, rule=None):
    """eval_apk.m for one part: score (n,), fr (n,) 0-based frames, point (n, 2), the frames' instances as in the contract"""
    si = m_sort(score, descend=True)
    numca = len(si)
    tp = np.zeros(numca); fp = np.zeros(numca)
    det = np.zeros(int(gt_offset[-1]), bool)
    for n, k in enumerate(si):
        i = fr[k]
        g0, g1 = int(gt_offset[i]), int(gt_offset[i + 1])
        if g1 == g0:
            fp[n] = 1
            continue
        with np.errstate(all="ignore"):
            dist = np.sqrt(((point[k][None, :] - gt_point[g0:g1, part]) ** 2).sum(1)) / gt_scale[g0:g1]
        if np.isnan(dist).all():
            fp[n] = 1
            continue
        distmin = np.nanmin(dist)
        js = np.flatnonzero(dist == distmin)
        jmin = g0 + int(js[-1] if rule == "last_jmin" else js[0])
        near = distmin < thresh if rule == "lt" else distmin <= thresh
        if near and not det[jmin]:
            tp[n] = 1
            det[jmin] = True
        else:
            fp[n] = 1
    fp = np.cumsum(fp); tp = np.cumsum(tp)
    rec = tp / float(gt_offset[-1])
    prec = tp / (fp + tp)
    return m_vocap(rec, prec, rule), prec, rec


# ---- part NMS ----------------------------------------------------------------------------------------------------------------
NPARTS = [1, 2, 26]


def literal_nms(rec, nparts, overlap, max_boxes, rule=None):
    return rec[m_nms(box_matrix(rec, nparts), float(np.float32(overlap)), nparts, max_boxes, rule)]


def all_nms_cases():
    for nparts in NPARTS:
        for name, overlap, max_boxes, rows, kept in H.nms_cases(nparts):
            yield nparts, name, overlap, max_boxes, H.records(nparts, rows), kept
    for seed, n, max_boxes in [(1, 40, 1000), (2, 300, 1000), (3, 300, 25), (4, 1200, 1000)]:
        yield 2, f"random{seed}", 0.3, max_boxes, H.random_records(seed, n, 2, 0, span=200), None
    yield 26, "random26", 0.3, 1000, H.random_records(5, 150, 26, 0, span=150), None


@pytest.mark.parametrize("nparts", NPARTS)
def test_nms_cases_reach_what_they_promise(nparts):
    for name, overlap, max_boxes, rows, kept in H.nms_cases(nparts):
        rec = H.records(nparts, rows)
        got = ev.nms_frame(rec, nparts, overlap, max_boxes)
        assert got.tobytes() == rec[kept].tobytes(), name


def test_nms_yardstick_equals_the_literal_file():
    ncut = 0
    for nparts, name, overlap, max_boxes, rec, _ in all_nms_cases():
        want = literal_nms(rec, nparts, overlap, max_boxes)
        got = ev.nms_frame(rec, nparts, overlap, max_boxes)
        assert got.tobytes() == want.tobytes(), (nparts, name)
        ncut += len(rec) > max_boxes
        assert 0 < len(got) <= min(len(rec), max_boxes)
    assert ncut >= 4


@pytest.mark.parametrize("rule", ["other_area", "product", "ge", "tie_first"])
def test_nms_every_rule_matters(rule):
    differ = [name for nparts, name, overlap, max_boxes, rec, _ in all_nms_cases()
              if literal_nms(rec, nparts, overlap, max_boxes, rule).tobytes() != ev.nms_frame(rec, nparts, overlap, max_boxes).tobytes()]
    assert differ, rule
    expect = {"other_area": "large_then_small", "product": "division_not_product", "ge": "o_equals_half", "tie_first": "tie_overlapping"}
    assert expect[rule] in differ


def test_division_case_is_what_the_search_found():
    """inter / area > 0.3f and inter > 0.3f * area disagree on the kept case (double arithmetic, one rounding per operation)"""
    (_, _, a), (_, _, b) = H.nms_cases(1)[2][3]
    inter = np.float64(b[0][2] + 1) * np.float64(b[0][3] + 1)
    area = np.float64(a[0][2] + 1) * np.float64(a[0][3] + 1)
    assert not inter / area > H.OV03 and inter > H.OV03 * area
    assert inter / area == H.OV03                       # the quotient rounds onto the threshold


def test_cut_order_cannot_be_seen():
    """nms.m reorders a cut list (boxes(I(1:1000), :)).  The contract says so and the yardstick does so, but no output can show it:
    the stable descending sort leaves equal scores in list order, which is the order they have in the uncut list, so `sort(s)`
    taken from the end breaks ties the same way in both.  A cut that keeps the survivors in list order therefore gives the same
    picks on every list; this is asserted here instead of a case on which the two would differ, which cannot exist."""
    for nparts, name, overlap, max_boxes, rec, _ in all_nms_cases():
        assert literal_nms(rec, nparts, overlap, max_boxes, "cut_keeps_list_order").tobytes() == \
            literal_nms(rec, nparts, overlap, max_boxes).tobytes(), name
    # what the cut does show: without it more records survive
    rec = H.random_records(3, 300, 2, 0, span=200)
    assert len(ev.nms_frame(rec, 2, 0.3, 25)) < len(ev.nms_frame(rec, 2, 0.3, 1000))


def test_nms_many_frames_and_nan_scores():
    rec, nframes = H.nms_many_frames(2, frame_offset=3)
    out = ev.part_nms(rec, nframes, 2, 0.3, 1000, frame_offset=3)
    assert np.all(np.diff(out[:, 0]) >= 0) and 0 < len(out) < len(rec)
    one = H.records(1, [(0, float("nan"), H.same(1, 0, 0, 9, 9)), (0, 1.0, H.same(1, 50, 0, 9, 9)), (0, float("nan"), H.same(1, 100, 0, 9, 9))])
    assert ev.nms_frame(one, 1, 0.3).tobytes() == one[[1, 0, 2]].tobytes()      # NaN last, in list order
    assert ev.nms_frame(one, 1, 0.3, 2).tobytes() == one[[1, 0]].tobytes()


# ---- best overlap ------------------------------------------------------------------------------------------------------------
def literal_best(rec, nparts, gt, overlap, rule=None):
    out = []
    for f in range(len(gt)):
        idx = np.flatnonzero(rec[:, 0] == f)
        idx = idx[~np.isnan(ev.scores(rec)[idx])]          # project decision, not Matlab's: a NaN score is never chosen
        g = None if np.isnan(gt[f]).any() else gt[f] + 1.0
        k = m_bestoverlap(box_matrix(rec[idx], nparts), g, float(np.float32(overlap)), rule)
        out.append(None if k is None else int(idx[k]))
    return out


@pytest.mark.parametrize("nparts", [2, 26])
def test_best_overlap(nparts):
    rows, gt, overlap, chosen = H.best_cases(nparts)
    rec = H.records(nparts, rows)
    out, found = ev.best_overlap(rec, len(gt), nparts, gt, overlap)
    assert found.tolist() == [int(c is not None) for c in chosen]
    for f, c in enumerate(chosen):
        assert out[f].tobytes() == (rec[c] if c is not None else np.zeros_like(rec[0])).tobytes(), f
    assert literal_best(rec, nparts, gt, overlap) == chosen
    assert literal_best(rec, nparts, gt, overlap, "ge") != chosen
    assert literal_best(rec, nparts, gt, overlap, "tie_last") != chosen
    # a frame offset, and a long list
    rec9 = rec.copy()
    rec9[:, 0] += 9
    out9, found9 = ev.best_overlap(rec9, len(gt), nparts, gt, overlap, frame_offset=9)
    assert found9.tolist() == found.tolist() and out9[:, 1:].tobytes() == out[:, 1:].tobytes()


# ---- PCK ---------------------------------------------------------------------------------------------------------------------
def test_pck():
    rows, found, gt, scale, thresh, pck = H.pck_case(2)
    rec = H.records(2, rows)
    got, dist = ev.eval_pck(rec, found, 2, gt, scale, thresh)
    assert got.tolist() == pck.tolist()
    assert dist[1, 0] == 5.0 and np.isinf(dist[0, 2]) and np.isnan(dist[0, 3])
    # against the file: every frame found, one scale (the file uses the last frame's for all), no NaN
    rec = H.random_records(7, 30, 2, 0, span=40)
    gtp = np.round(ev.centres(rec, 2) + 3.0 * np.sin(np.arange(120.0)).reshape(30, 2, 2))
    gtp[0] = ev.centres(rec, 2)[0] + np.array([3.0, 4.0])            # dist == thresh * scale
    sc = np.full(30, 10.0)
    got, dist = ev.eval_pck(rec, np.ones(30, np.int32), 2, gtp, sc, 0.5)
    want, wdist = m_eval_pck(ev.centres(rec, 2) + 1.0, gtp + 1.0, 10.0, 0.5)
    assert got.tobytes() == want.tobytes() and dist.tobytes() == wdist.tobytes() and 0 < got.min() and got.max() < 1
    assert m_eval_pck(ev.centres(rec, 2) + 1.0, gtp + 1.0, 10.0, 0.5, "le")[0].tobytes() != got.tobytes()


# ---- APK ---------------------------------------------------------------------------------------------------------------------
def literal_apk(rec, nparts, gt_offset, gt, gs, thresh, rule=None, frame_offset=0):
    c = ev.centres(rec, nparts)
    s = ev.scores(rec).astype(np.float64)
    fr = rec[:, 0].astype(np.int64) - frame_offset
    res = [m_eval_apk(s, fr, c[:, p] + 1.0, gt_offset, gt + 1.0, gs, thresh, p, rule) for p in range(nparts)]
    return (np.array([r[0] for r in res]), np.array([r[1] for r in res]).reshape(nparts, -1),
            np.array([r[2] for r in res]).reshape(nparts, -1))


APK_CASES = [H.apk_case, H.apk_first_jmin_case, H.apk_sum_order_case]


@pytest.mark.parametrize("case", APK_CASES)
def test_apk_cases_reach_what_they_promise(case):
    rows, gt_offset, gt, gs, thresh, tp = case(2)
    rec = H.records(2, rows)
    apk, prec, rcl = ev.eval_apk(rec, len(gt_offset) - 1, 2, gt_offset, gt, gs, thresh)
    tpcum = np.cumsum(tp)
    assert prec[0].tolist() == (tpcum / np.arange(1, len(tp) + 1)).tolist()
    assert rcl[0].tolist() == (tpcum / float(gt_offset[-1])).tolist()
    want = literal_apk(rec, 2, gt_offset, gt, gs, thresh)
    assert apk.tobytes() == want[0].tobytes() and prec.tobytes() == want[1].tobytes() and rcl.tobytes() == want[2].tobytes()


def test_apk_sum_order_value():
    rows, gt_offset, gt, gs, thresh, _ = H.apk_sum_order_case(2)
    apk = ev.eval_apk(H.records(2, rows), 1, 2, gt_offset, gt, gs, thresh)[0]
    assert apk[0] == 0.9166666666666666 and apk[0] != 0.9166666666666665


@pytest.mark.parametrize("rule,case", [("last_jmin", H.apk_first_jmin_case), ("lt", H.apk_case), ("descending_sum", H.apk_sum_order_case)])
def test_apk_every_rule_matters(rule, case):
    rows, gt_offset, gt, gs, thresh, _ = case(2)
    rec = H.records(2, rows)
    assert literal_apk(rec, 2, gt_offset, gt, gs, thresh, rule)[0].tobytes() != \
        ev.eval_apk(rec, len(gt_offset) - 1, 2, gt_offset, gt, gs, thresh)[0].tobytes()


def test_apk_random_and_empty():
    rec, gt_offset, gt, gs = H.apk_random(21, 400, 2, frame_offset=5)
    got = ev.eval_apk(rec, len(gt_offset) - 1, 2, gt_offset, gt, gs, 0.5, frame_offset=5)
    nonan = ~np.isnan(ev.scores(rec))
    want = literal_apk(rec[nonan], 2, gt_offset, gt, gs, 0.5, frame_offset=5)
    got_nonan = ev.eval_apk(rec[nonan], len(gt_offset) - 1, 2, gt_offset, gt, gs, 0.5, frame_offset=5)
    for a, b in zip(got_nonan, want):
        assert a.tobytes() == b.tobytes()
    assert 0 < got[0].min() and got[0].max() < 1
    empty = ev.eval_apk(rec[:0], len(gt_offset) - 1, 2, gt_offset, gt, gs, 0.5)
    assert empty[0].tolist() == [0.0, 0.0] and empty[1].shape == (2, 0)


# ---- the layers above the kernels --------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from partsbaseddetector_amd import _lib, build
    build.build_hip()
    lib = _lib.load()
    names = ["pbd_part_nms", "pbd_best_overlap", "pbd_eval_pck", "pbd_eval_apk"]
    for n in names + [n + "_device" for n in names]:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    for k in ("k_ev_nms_select", "k_ev_nms_pairs", "k_ev_nms_greedy", "k_ev_nms_emit", "k_ev_best", "k_ev_pck", "k_ev_apk_rank",
              "k_ev_apk_close", "k_ev_apk_ap"):
        assert lib.pbd_kernel_name(_lib.KERNELS.index(k)).decode() == k


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_members_compile(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
size_t use(pbdhost::PartsBasedDetector<T> &d, const std::vector<pbdhost::Candidate> &c)
{
    std::vector<pbdhost::Candidate> kept = d.partNMS(c, 2, 0.3f, 1000);
    std::vector<double> gtbox(8, 0.0), pts(2 * 26 * 2, 0.0), scale(2, 1.0);
    std::vector<pbdhost::Candidate> best;
    std::vector<bool> found;
    d.bestOverlap(c, gtbox, 0.3f, best, found);
    std::vector<double> dist;
    std::vector<double> pck = d.evalPCK(best, found, pts, scale, 0.5, &dist);
    std::vector<int32_t> gt_offset(3, 0);
    std::vector<double> prec, rec;
    std::vector<double> apk = d.evalAPK(kept, gt_offset, pts, scale, 0.5, &prec, &rec);
    return kept.size() + pck.size() + apk.size() + dist.size() + prec.size() + rec.size();
}
template size_t use<float>(pbdhost::PartsBasedDetector<float> &, const std::vector<pbdhost::Candidate> &);
template size_t use<double>(pbdhost::PartsBasedDetector<double> &, const std::vector<pbdhost::Candidate> &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
