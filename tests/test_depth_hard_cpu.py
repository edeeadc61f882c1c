"""The built hard depth images (tests/depth_hard_images.py) keep their promises, on the CPU: every consistency case gets the
promised keep bit from consistency.keep_record and from a brute-force sorted()[M // 2]; every 3-D box case has
Candidate.boundingBox3D equal to the scalar restatement slow_box3d bit for bit; the coverage the cases are built for is asserted,
so a later edit cannot hollow them out; and plain numpy replays of the two select schemes (k_boxes3d: 4-bit passes, one histogram
row per key prefix, residual ranks; dc_select: 8-bit passes with a prefix match) reproduce every expectation, while each named
mutation of a replay changes the expected output of at least one built case.  No GPU."""
import functools

import numpy as np
import pytest

import depth_hard_images as H
from test_boxes3d_cpu import bits, cand, slow_box3d
from partsbaseddetector_amd import consistency
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import _dog_filter_400, _rect_and, _walk_400

F32, F64 = np.float32, np.float64
REALS = (F32, F64)


# ---- depth consistency: promises -----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def dc_cases():
    return H.consistency_cases()


@functools.lru_cache(None)
def two_part_flat():
    return M.synthetic_model(seed=5, pa=[0, 1], nmix=1, name="two").flatten()


def brute_keep(img, c, T):
    """the decision from a sorted list, no np.partition: part boxes clipped by hand, the rows cast to T, NaN read as 0"""
    def box_samples(b):
        x, y, w, h = b
        out = []
        for yy in range(max(y, 0), min(y + h, img.shape[0])):
            with np.errstate(over="ignore"):
                row = img[yy, max(x, 0):min(x + w, img.shape[1])].astype(T)
            out += [T(0) if v != v else v for v in row]
        return out
    ch, pa = box_samples(c.box), box_samples(c.parent)
    assert len(ch) == c.M and len(pa) == 1
    mc, mq = sorted(ch)[c.M // 2], pa[0]
    if not (mc > 0 and mq > 0):
        return True
    with np.errstate(invalid="ignore", over="ignore"):
        d = abs(T(mc) - T(mq))
    return not d > 0


@pytest.mark.parametrize("code", ["u8", "u16", "f32", "f64"])
def test_consistency_cases_keep_their_promise(code):
    img, cases = dc_cases()[code]
    flat = two_part_flat()
    norms = consistency.anchor_norms(flat)
    assert norms[1] > 0                                           # the threshold norm * 0 is a plain 0
    for T in REALS:
        sel = [c for c in cases if T in c.keeps]
        rec = H.dc_records(sel, 16)
        for c, r in zip(sel, rec):
            assert consistency.keep_record(flat, r, img, 0.0, T, norms) == c.keeps[T], (c.name, T.__name__)
            assert brute_keep(img, c, T) == c.keeps[T], (c.name, T.__name__)
        kept = consistency.filter_records(flat, rec, [img], 0.0, T)
        assert np.array_equal(kept, rec[[c.keeps[T] for c in sel]])
        assert 0 < len(kept) < len(rec)


def test_restated_constants_are_the_kernels():
    """the sizes the builders restate, read from the constexpr lines of the kernel sources: if one changes, the cases built to
    cross it must move with it"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "partsbaseddetector_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("pbd_internal.h", "pbd_kernels_consistency.hip", "pbd_kernels_depth.hip"))

    def const(name):
        m = re.findall(r"constexpr int " + name + r" = (\d+);", text)
        assert len(m) == 1, name
        return int(m[0])

    assert (const("kDcWaveKeys"), const("kDcBlockKeys")) == (H.WAVE_KEYS, H.BLOCK_KEYS)
    assert (const("kDcMaxGrid"), const("kDcThreads"), const("kB3MaxGrid"), const("kB3Out")) == \
        (H.DC_MAX_GRID, H.DC_THREADS, H.B3_MAX_GRID, H.B3_OUT)
    # the three select grids as launch_dc_select writes them
    assert re.search(r"g0 = std::max\(std::min\(ntask, kDcMaxGrid \* 4\), 1\), g1 = std::max\(std::min\(ntask, kDcMaxGrid\), 1\);", text)
    assert re.search(r"g2 = std::max\(std::min\(ntask, kDcMaxGrid / 4\), 1\);", text)


def test_consistency_coverage():
    """every size class x depth code x real type has an exact (kept), a below and an above (dropped) case; the class edges, the
    widths and the clipped boxes are all there"""
    all_cases = [c for code in dc_cases() for c in dc_cases()[code][1]]
    for code in ("u8", "u16", "f32", "f64", "f64f", "f64m"):
        for T in REALS:
            for cls in range(3):
                for variant, keep in (("exact", True), ("below", False), ("above", False)):
                    hit = [c for c in all_cases if c.code == code and c.cls == cls and c.variant == variant and c.keeps.get(T) is keep]
                    if code == "f64" and T == F32 and not keep:
                        continue                                  # double-ulp neighbours are one float: nothing drops (f64f does)
                    assert hit, (code, T.__name__, cls, variant)
            for variant in ("decoy-exact", "decoy-below", "decoy-above"):
                if code == "f64" and T == F32 or code == "f64m":
                    continue
                assert {c.cls for c in all_cases if c.code == code and c.variant == variant and T in c.keeps} == {0, 1, 2}
    ms = {c.M for c in all_cases}
    assert {1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4900, 20000, 20022} <= ms
    assert {63 * 70, 30 * 20, 65 * 17} <= ms                      # the clipped areas
    img = dc_cases()["f32"][0]
    assert any(c.box[0] < 0 for c in all_cases) and any(c.box[0] + c.box[2] > H.DC_W for c in all_cases)
    assert any(c.box[1] + c.box[3] > img.shape[0] for c in dc_cases()["f32"][1])
    # under T = float the double-ulp neighbours keep regardless: the stated exception
    f64 = [c for c in dc_cases()["f64"][1] if c.code == "f64" and c.name.startswith("f64-A") and c.variant in ("below", "above")]
    assert f64 and all(c.keeps[F32] and not c.keeps[F64] for c in f64 if c.M > 2)
    # distinct doubles that are one float on one side: the median drops under both real types, through different keys
    f64m = [c for c in all_cases if c.code == "f64m" and c.variant == "above"]
    assert f64m and not any(c.keeps[F32] or c.keeps[F64] for c in f64m)
    # Inf against Inf keeps (Inf - Inf is NaN)
    assert any("inf" in c.name and c.variant == "exact" and c.keeps[F32] for c in all_cases)


def test_long_and_emit_lists():
    img, cases = dc_cases()["f32"]
    probes = H.probe_cases(cases, F32)
    assert [c.keeps[F32] for c in probes] == [True, False] * 3 and {c.cls for c in probes} == {0, 1, 2}
    n = 40400
    rec, which = H.long_list(probes, 8 + 4 * 26, 26, n, dense_from=40320)
    assert n * 26 > H.DC_MAX_GRID * H.DC_THREADS                 # k_dc_classify's second trip
    first_second = H.DC_MAX_GRID * H.DC_THREADS // 26             # the record the 2^20-th task belongs to
    assert (which[first_second - 8:] >= 0).all() and (which >= 0).sum() > 400
    assert {bool(probes[k].keeps[F32]) for k in which[first_second:]} == {True, False}
    rec2, pattern = H.emit_list(probes, F32, 16)
    assert len(rec2) > 5 * H.DC_THREADS
    per_block = [int(pattern[b:b + H.DC_THREADS].sum()) for b in range(0, len(pattern), H.DC_THREADS)]
    assert len(set(per_block)) > 3 and pattern[255] and pattern[256] and pattern[767] and pattern[768]
    kept = consistency.filter_records(two_part_flat(), rec2, [img], 0.0, F32)
    assert np.array_equal(kept, rec2[pattern])


@pytest.mark.parametrize("T", REALS)
def test_reentry_list(T):
    """each size class holds more medians than its select launch has workgroups, kept and dropped records in each"""
    img, cases = dc_cases()["f32"]
    rec, keep = H.reentry_list(cases, T, 16)
    assert len(rec) * 2 > H.DC_SELECT_GRIDS[0]                    # ntask, which caps every grid, is above the largest
    cls = np.array([H.size_class(int(r[14]) * int(r[15])) for r in rec])      # all these child boxes lie inside the image
    tasks = [len(rec) + int((cls == 0).sum()), int((cls == 1).sum()), int((cls == 2).sum())]   # the 1 x 1 parents are class 0
    assert all(t > g for t, g in zip(tasks, H.DC_SELECT_GRIDS)), tasks
    for k in range(3):
        assert {bool(v) for v in keep[cls == k]} == {True, False}
        assert len({tuple(r[12:16]) for r in rec[cls == k]}) >= 12      # many different medians per class
    kept = consistency.filter_records(two_part_flat(), rec, [img], 0.0, T)
    assert np.array_equal(kept, rec[keep])


# ---- 3-D boxes: promises ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def b3_sets():
    """{set name: (frames, cases)} of every 3-D box builder; the long lists reduced to their distinct records"""
    sets = {"sweeps": H.boxes3d_sweeps()}
    for code in ("u8", "u16", "f64"):
        sets[code] = H.boxes3d_coded(code)
    frames, cases = H.boxes3d_long_list(False)
    seen, uniq = set(), []
    for c in cases:
        k = (c.frame, tuple(map(tuple, c.parts)))
        if k not in seen:
            seen.add(k)
            uniq.append(c)
    sets["long"] = (frames, uniq)
    return sets


@functools.lru_cache(None)
def b3_steps(name):
    frames, cases = b3_sets()[name]
    return [cand(c.parts).boundingBox3D_steps(frames[c.frame].shape, frames[c.frame]) for c in cases]


@functools.lru_cache(None)
def b3_mirror(name):
    frames, cases = b3_sets()[name]
    return [cand(c.parts).boundingBox3D(frames[c.frame].shape, frames[c.frame]) for c in cases]


@pytest.mark.parametrize("name", ["sweeps", "u8", "u16", "f64", "long"])
def test_boxes3d_mirror_equals_scalar_restatement(name):
    frames, cases = b3_sets()[name]
    for c, want in zip(cases, b3_mirror(name)):
        d = frames[c.frame]
        assert (bits(want) == bits(slow_box3d([list(p) for p in c.parts], d.shape[0], d.shape[1], d))).all(), c.name


def test_boxes3d_coverage():
    frames, cases = b3_sets()["sweeps"]
    steps = b3_steps("sweeps")
    lo, hi, lo150, hi150 = set(), set(), set(), set()
    for c, st in zip(cases, steps):
        if c.kind != "sweep":
            continue
        assert len(st["S"]) == c.M, c.name
        (lo if c.M >= 400 else lo150).add(st["dmin"])
        (hi if c.M >= 400 else hi150).add(st["dmax"])
    assert len(lo & set(range(0, 201))) >= 185 and len(hi & set(range(200, 400))) >= 185, (len(lo), len(hi))
    assert len(lo150) >= 60 and len(hi150) >= 60, (len(lo150), len(hi150))
    assert {400, 401, 799, 800, 801, 150, 2, 1013, 4000, 70000} <= {c.M for c in cases}
    kinds = {c.name.split("-")[1] for c in cases if c.kind == "sweep"}
    assert kinds == {"bits", "lin", "zero"}
    widths = {c.parts[0][2] for c in cases if c.kind == "sweep"}
    assert {1, 63, 64, 65, 129} <= widths
    assert {c.parts[0][3] < 16 for c in cases if c.kind == "sweep"} == {True, False}
    by = {c.name: st for c, st in zip(cases, steps)}
    for m in (150, 400, 801):                                     # the denormal records: the walk runs to both ends, over denormals
        st = by[f"M{m}-denorm"]
        assert (st["dmin"], st["dmax"]) == (0, 399) and 0 < st["p"][0] < np.finfo(F32).tiny and 0 < st["p"][399] < np.finfo(F32).tiny
    assert by["nanbox"] is None and by["holes-second"] is not None
    assert len(by["multibox-300"]["S"]) > 40 * 30                 # the overlaps and the boundingBoxNorm box count again
    # the other depth codes: the walk ends at many different rows, and 64F samples are not floats
    for code in ("u8", "u16", "f64"):
        ends = {(st["dmin"], st["dmax"]) for st in b3_steps(code)}
        assert len(ends) >= 20, (code, len(ends))
    # the long list: more than the grid, and the two records of one workgroup pair every kind with every other
    for device, nk in ((False, 5), (True, 6)):
        _, long_cases = H.boxes3d_long_list(device)
        assert len(long_cases) > H.B3_MAX_GRID
        pairs = {(long_cases[i].kind, long_cases[i + H.B3_MAX_GRID].kind) for i in range(len(long_cases) - H.B3_MAX_GRID)}
        assert len(pairs) == nk * nk


# ---- the select schemes replayed ---------------------------------------------------------------------------------------------------
def f32_keys(v, mut):
    """float_key of float32 samples (as uint32)"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    if mut == "noflip":
        return b | np.uint32(0x80000000)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def f32_unkey(k, mut):
    k = np.asarray(k, np.uint32)
    if mut == "noflip":
        return (k & np.uint32(0x7fffffff)).view(F32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(F32)


def flush32(v):
    v = np.array(v, F32)
    v[np.abs(v) < np.finfo(F32).tiny] = 0
    return v


def replay_box3d(c, depth, mut=None, mut_pass=None):
    """k_boxes3d's scheme in numpy: the boxes' samples, pass 0 counting M and the first box's valid samples, the needed ranks
    merged, eight 4-bit passes with one histogram row per distinct prefix and a residual rank per needed rank, then the
    resample from the resolved keys.  The filter and the walk are the yardstick's."""
    ca = cand(c.parts)
    rows, cols = depth.shape
    boxes = [_rect_and(tuple(int(v) for v in r), (0, 0, cols, rows)) for r in ca.parts]
    boxes.append(_rect_and(ca.boundingBoxNorm(), (0, 0, cols, rows)))
    boxes = [b for b in boxes if b[2] > 0 and b[3] > 0]           # the colour frame has the depth image's shape: scale 1
    nan_box = (np.nan, np.nan, np.nan, 0.0, 0.0, 0.0)
    if not boxes:
        return nan_box
    per_box = []
    for x, y, w, h in boxes:
        v = depth[y:y + h, x:x + w].astype(F32).ravel()
        if mut == "flush":
            v = flush32(v)
        ok = v != 0
        if mut != "nan_kept":
            ok &= ~np.isnan(v)
        per_box.append(v[ok])
    vals = np.concatenate(per_box)
    Mn = vals.size
    first_valid = Mn if mut == "first_valid_all" else per_box[0].size
    if first_valid == 0 or Mn == 0:
        return nan_box
    keys = f32_keys(vals, mut)
    # the needed ranks
    if Mn == 400:
        sy, fy = np.arange(400), None
    else:
        f = ((np.arange(400) + 0.5) * (1.0 / (400.0 / Mn)) - 0.5).astype(F32)
        sy = np.floor(f).astype(np.int64)
        fy = (f - sy.astype(F32)).astype(F32)
    r0, r1 = np.clip(sy, 0, Mn - 1), np.clip(sy + 1, 0, Mn - 1)
    rank = np.unique(np.concatenate([r0, r1]))
    pre = np.zeros(len(rank), np.uint32)
    resid = np.minimum(rank + 1, Mn - 1) if mut == "rank_off" else rank.copy()
    for p in range(8):
        shift = 28 - 4 * p
        if mut == "skip_last" and p == 7:
            pre = pre << np.uint32(4)
            break
        upre = np.unique(pre)                                     # the rows: one per distinct prefix
        kp = (keys.astype(np.uint64) >> np.uint64(shift + 4)).astype(np.uint32)
        digit = ((keys >> np.uint32(shift)) & np.uint32(15)).astype(np.int64)
        if mut == "prefix_dropped" and p == mut_pass:
            hist = np.tile(np.bincount(digit, minlength=16), (len(upre), 1))
        else:
            row = np.searchsorted(upre, kp)
            hit = (row < len(upre)) & (upre[np.minimum(row, len(upre) - 1)] == kp)
            hist = np.bincount(row[hit] * 16 + digit[hit], minlength=16 * len(upre)).reshape(len(upre), 16)
        my = np.searchsorted(upre, pre)
        cum = np.cumsum(hist[my], axis=1)
        dg = np.minimum((cum <= resid[:, None]).sum(axis=1), 15)
        resid = resid - np.where(dg > 0, cum[np.arange(len(rank)), np.maximum(dg - 1, 0)], 0)
        pre = (pre << np.uint32(4)) | dg.astype(np.uint32)
    val = f32_unkey(pre, mut)
    s0, s1 = val[np.searchsorted(rank, r0)], val[np.searchsorted(rank, r1)]
    with np.errstate(invalid="ignore", over="ignore"):
        if Mn == 400:
            pts = s0
        else:
            w1 = fy.copy()
            if mut == "reset_weights":                            # cv::resize's x direction does this at the clamp; y does not
                w1[(sy < 0) | (sy >= Mn - 1)] = 0
            pts = s0 * (F32(1) - w1) + s1 * w1
    dmin, dmax = _walk_400(_dog_filter_400(pts))
    bx, by, bw, bh = ca.boundingBox()
    return float(bx), float(by), float(pts[dmin]), float(bh), float(bw), float(pts[dmax]) - float(pts[dmin])


def dc_keys(img, box, code, T, mut):
    """dc_key of a clipped part box: (uint64 keys, key bits)"""
    s = img[max(box[1], 0):box[1] + box[3], max(box[0], 0):box[0] + box[2]].ravel()
    kb = H.key_bits(H.image_code(code), T)
    if code in ("u8", "u16"):
        return s.astype(np.uint64), kb
    if kb == 64:
        v = s.astype(F64)
        if mut == "flush":
            v[np.abs(v) < np.finfo(F64).tiny] = 0
        if mut != "nan_kept":
            v[np.isnan(v)] = 0
        v = v + 0.0
        b = v.view(np.uint64)
        if mut == "noflip":
            return b | np.uint64(1 << 63), kb
        return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63)), kb
    with np.errstate(over="ignore"):
        v = s.astype(F32)
    if mut == "flush":
        v = flush32(v)
    if mut != "nan_kept":
        v[np.isnan(v)] = 0
    return f32_keys(v + F32(0), mut).astype(np.uint64), kb


def dc_unkey(k, code, kb, mut):
    if code in ("u8", "u16"):
        return float(k)
    if kb == 64:
        k = np.uint64(k)
        if mut == "noflip":
            return float(np.array(k & np.uint64((1 << 63) - 1)).view(F64))
        return float(np.array(k & np.uint64((1 << 63) - 1) if k >> np.uint64(63) else ~k).view(F64))
    return float(f32_unkey(np.array([k], np.uint32), mut)[0])


def replay_select(keys, kb, rank, mut=None, mut_pass=None):
    """dc_select: kb / 8 passes of 8 bits; a key is counted when the bits above the pass's digit match the prefix so far"""
    prefix, rem = 0, rank
    npass = kb // 8
    for p in range(npass):
        shift = kb - 8 * (p + 1)
        hs = shift + 8
        if mut == "skip_last" and p == npass - 1 and npass > 1:
            break
        if hs >= kb or (mut == "prefix_dropped" and p == mut_pass):
            match = np.ones(len(keys), bool)
        else:
            match = (keys >> np.uint64(hs)) == np.uint64(prefix >> hs)
        hist = np.bincount(((keys[match] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        cum = np.cumsum(hist)
        d = min(int((cum <= rem).sum()), 255)
        rem -= int(cum[d - 1]) if d else 0
        prefix |= d << shift
    return prefix


def replay_keep(img, c, T, mut=None, mut_pass=None):
    """k_dc_decide on the replayed medians, zfactor = 0"""
    med = []
    for box in (c.parent, c.box):
        keys, kb = dc_keys(img, box, c.code, T, mut)
        rank = len(keys) // 2
        if mut == "rank_off" and len(keys) > 1:
            rank = min(rank + 1, len(keys) - 1)
        med.append(dc_unkey(replay_select(keys, kb, rank, mut, mut_pass), c.code, kb, mut))
    mq, mc = med
    if mc != mc or mq != mq or not (mc > 0 and mq > 0):
        return True
    with np.errstate(invalid="ignore", over="ignore"):
        d = abs(F64(mc) - F64(mq)) if T == F64 else F64(abs(F32(mc) - F32(mq)))
    return not d > 0


def dc_all():
    return [(dc_cases()[img_code][0], c) for img_code in dc_cases() for c in dc_cases()[img_code][1]]


def test_consistency_replay_reproduces_every_promise():
    for img, c in dc_all():
        for T in c.keeps:
            assert replay_keep(img, c, T) == c.keeps[T], (c.name, T.__name__)


DC_MUTATIONS = [("rank_off", None), ("skip_last", None), ("noflip", None), ("flush", None), ("nan_kept", None)] + \
    [("prefix_dropped", p) for p in range(1, 8)]


@pytest.mark.parametrize("mut,mut_pass", DC_MUTATIONS)
def test_consistency_mutation_is_caught(mut, mut_pass):
    """each mutation of the replay flips the keep bit of a built case, in every key width it applies to and under both real types"""
    for T in REALS:
        for kb in (8, 16, 32, 64):
            npass = kb // 8
            if kb == 64 and T == F32:
                continue
            if mut == "prefix_dropped" and mut_pass >= npass:
                continue
            if kb in (8, 16) and mut in ("noflip", "flush", "nan_kept") or kb == 8 and mut == "skip_last":
                continue                                          # integer keys have no sign, denormal or NaN; one pass is the last
            caught = []
            for img, c in dc_all():
                if T in c.keeps and H.key_bits(H.image_code(c.code), T) == kb and c.M <= 5000:
                    if replay_keep(img, c, T, mut, mut_pass) != c.keeps[T]:
                        caught.append(c.name)
                        break
            assert caught, (mut, mut_pass, T.__name__, kb)


def b3_ordered():
    """(set name, index) of the 3-D box cases, the special records first so that a mutation's search ends early"""
    out = []
    for name in ("sweeps", "f64", "u8", "long"):
        cases = b3_sets()[name][1]
        out += [(c.kind == "sweep", name, i) for i, c in enumerate(cases) if c.M is None or c.M <= 5000]
    return [(n, i) for _, n, i in sorted(out, key=lambda t: t[0])]


@pytest.mark.parametrize("name", ["sweeps", "u8", "u16", "f64", "long"])
def test_boxes3d_replay_reproduces_every_box(name):
    frames, cases = b3_sets()[name]
    for c, want in zip(cases, b3_mirror(name)):
        assert (bits(replay_box3d(c, frames[c.frame])) == bits(want)).all(), c.name


B3_MUTATIONS = [("rank_off", None), ("skip_last", None), ("noflip", None), ("flush", None), ("nan_kept", None),
                ("first_valid_all", None), ("reset_weights", None)] + [("prefix_dropped", p) for p in range(1, 8)]


@pytest.mark.parametrize("mut,mut_pass", B3_MUTATIONS)
def test_boxes3d_mutation_is_caught(mut, mut_pass):
    for name, i in b3_ordered():
        frames, cases = b3_sets()[name]
        c = cases[i]
        if (bits(replay_box3d(c, frames[c.frame], mut, mut_pass)) != bits(b3_mirror(name)[i])).any():
            return
    pytest.fail(f"no built case notices {mut} {mut_pass}")
