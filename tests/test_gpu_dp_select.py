"""The selection half of pbd_kernels_dp.hip -- k_dp_combine (every MAXM bucket x fp32 / fp64 / fp16 responses x uint8 / int16
position planes), k_dp_combine_seq, k_dp_root, k_argmin_count / _scan / _emit and the four forms of k_argmin_walk -- against
the oracle, bit for bit, through the staged entry points pbd_dp_min and pbd_dp_argmin.

The inputs (tests/dp_hard_models.py) are what ordinary data never is: parts that differ in their number of mixtures, planes on
a power-of-two grid that tie exactly between mixtures, root scores equal to the threshold, scales that put rectangle corners on
exact halves, a level of more than 2^20 root scores, trees of 160 parts.  tests/test_dp_select_cpu.py checks the oracle against
a brute force on the same inputs and counts the ties, the threshold hits and the halves they hold.  No tolerances anywhere."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib
from partsbaseddetector_amd import synth

import dp_hard_models as D

pytestmark = pytest.mark.gpu

HANDLES = ("f32", "f64", "f16")


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


def _ksize(handle):
    return 5 if handle == "f16" else 3      # the matrix-core modes take 5 x 5 filters only; the staged entry points read none


def _handle(det_mod, flat, handle, **kw):
    kw.update({"f32": {}, "f64": {"real_type": _lib.REAL_F64}, "f16": {"conv_mode": _lib.CONV_MFMA_F16}}[handle])
    return det_mod.Handle(flat, device=0, **kw)


def _planes(model, dims, seed, handle):
    """what the handle is given and what the oracle is run on (fp16 responses: the planes rounded to fp16, which the grid
    survives unchanged)"""
    given = D.quantised_scores(model, dims, seed, np.float64 if handle == "f64" else np.float32)
    if handle == "f16":
        return given, [g.astype(np.float16).astype(np.float32) for g in given]
    return given, given


def _check_min(det_mod, oracle, model, handle, dims, seed):
    flat = model.flatten()
    given, ref_in = _planes(model, dims, seed, handle)
    bits = np.uint64 if handle == "f64" else np.uint32
    hd = _handle(det_mod, flat, handle)
    try:
        Ix, Iy, Ik, rootv, rooti = det_mod.DynamicProgram(hd).min(given)
    finally:
        hd.close()
    for l, s in enumerate(ref_in):
        for c in range(flat.ncomponents):
            oIx, oIy, oIk, orv, ori = oracle.dp_min(flat, c, s)
            where = (model.name, handle, l, dims[l], c)
            assert np.array_equal(rootv[l][c].view(bits), orv.view(bits)), where
            assert np.array_equal(rooti[l][c], ori), where
            p0, p1 = flat.part_offset[c], flat.part_offset[c + 1]
            for gp in range(p0 + 1, p1):
                par = p0 + flat.parentid[gp]
                for m in range(flat.mix_offset[par + 1] - flat.mix_offset[par]):
                    sl = flat.ptr_slot[gp] + m
                    assert np.array_equal(Ik[l][sl], oIk[sl]), where + (gp, m, "Ik")
                    assert np.array_equal(Ix[l][sl], oIx[sl]), where + (gp, m, "Ix")
                    assert np.array_equal(Iy[l][sl], oIy[sl]), where + (gp, m, "Iy")


# ---- combine and root ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name", list(D.SETS))
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("K", D.TABLE_K, ids=[f"mix{K}" for K in D.TABLE_K])
def test_combine_and_root_table(det_mod, oracle, K, handle, set_name):
    """Row K: tree [0, 1, 1, 2, 2] with mixtures [K, 1, K, max(K-1, 1), min(K, 2)] (two components for K = 2 and 8) -- the
    MAXM = 2 | 4 | 6 | 8 | 16 instantiation of k_dp_combine at both edges of its bucket, with a one-mixture child (the copy path),
    children below MAXM (the -inf padding) and one-mixture parents above them -- and k_dp_root over K accumulated planes."""
    _check_min(det_mod, oracle, D.table_model(K, _ksize(handle)), handle, D.SETS[set_name], 1000 + K)


def _refused(det_mod, model):
    """pbd_create on a model the library must refuse: its status, its handle, its message"""
    flat = model.flatten()
    lib = _lib.load()
    cm = _lib.c_model(flat)
    cfg = _lib.CConfig(0, _lib.REAL_F32, _lib.CONV_EXACT, 1, 1024, None)
    h = C.c_void_p()
    rc = lib.pbd_create(C.byref(cm), C.byref(cfg), C.byref(h))
    if h.value:
        lib.pbd_destroy(h)
    return rc, h.value, lib.pbd_last_error(None).decode()


def test_seventeen_mixtures_are_refused(det_mod):
    rc, h, msg = _refused(det_mod, D.mixed_model([2, 17], [0, 1], name="mix17"))
    assert rc == -2 and _lib.STATUS[rc] == "PBD_ERR_UNSUPPORTED" and not h and "17 mixtures" in msg, (rc, h, msg)
    with pytest.raises(_lib.PbdError) as e:
        det_mod.Handle(D.mixed_model([17], [0], name="root17"), device=0)
    assert e.value.code == -2


# ---- sequential schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name", list(D.SETS))
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("case", range(3))
def test_sequential_schedule(det_mod, oracle, case, handle, set_name):
    """The shared-filter cases of test_filter_shared_inside_a_component with two and three mixtures per part on the tying planes:
    k_dp_combine_seq's selection, and (f16) the fp16 read of an accumulator's first value."""
    _check_min(det_mod, oracle, D.shared_model(case, _ksize(handle)), handle, D.SETS[set_name], 300 + case)


# ---- root without children ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("K", [1, 2, 9])
def test_root_without_children(det_mod, oracle, K, handle):
    """k_dp_root reading raw responses (from_acc == 0), fp16 ones on the f16 handle; root mixtures tie"""
    for set_name in D.SETS:
        _check_min(det_mod, oracle, D.root_only_model(K, _ksize(handle)), handle, D.SETS[set_name], 50 + K)


# ---- find: order, threshold, the scan's second pass -------------------------------------------------------------------------------
FIND_SIDE = 364                             # 8 x 364 x 364 = 1 059 968 root scores: 1036 blocks of 1024, k_argmin_scan loops twice
FIND_THRESH = 0.5
FIND_BIAS = [0.0, -0.0, 0.0625, -0.0625, 0.25, -0.25, 0.125, 0.4375]


def _find_case(R):
    """model, responses (8, side, side) of R and the flat indices that must come back, in order"""
    model = D.mixed_model([[1]] * 8, [[0]] * 8, ncomponents=8, seed=8, thresh=FIND_THRESH, name="find")
    for c in range(8):
        model.biasw[model.biasid[c][0][0]] = FIND_BIAS[c]
    HW = FIND_SIDE * FIND_SIDE
    n = 8 * HW
    resp = np.full(n, -4.0, R)
    bias = np.repeat(np.asarray(FIND_BIAS, R), HW)
    t = R(np.float32(FIND_THRESH))
    above = np.nextafter(t, R(1))           # one ulp of R above the threshold: a hit (for R = double it rounds to the threshold as a float)

    def plant(i, value):
        resp[i] = R(value) - bias[i]
        assert resp[i] + bias[i] == R(value), (i, value)         # the root score is exactly `value`
    hits = []
    singles = [0, 255 * 4 - 1, 255 * 4 + 1, 1023, 1024, (1 << 20) - 1, 1 << 20, n - 1]
    for k, i in enumerate(singles):
        plant(i, 1.0 + k / 64.0)
        hits.append(i)
    start = 1024 * 517 - 150                # 300 consecutive cells across a block boundary, some of them no hits
    for k in range(300):
        i = start + k
        if k % 50 == 7:
            plant(i, t)                     # equal to the threshold: absent (strict >)
        elif k % 50 == 9:
            resp[i] = np.nan                # NaN compares false: absent
        elif k % 50 == 11:
            plant(i, above)
            hits.append(i)
        else:
            plant(i, 0.75 + (k % 32) / 128.0)
            hits.append(i)
    for c in range(8):                      # the three kinds under every component's bias
        i = c * HW + 5000 + 3 * c
        plant(i, t); plant(i + 1, above); resp[i + 2] = np.nan
        hits.append(i + 1)
    hits = np.array(sorted(hits))
    with np.errstate(invalid="ignore"):
        rootv = resp + bias
        assert np.array_equal(np.nonzero(rootv > t)[0], hits)       # the numpy reference of find
    return model, resp.reshape(8, FIND_SIDE, FIND_SIDE), hits, rootv


def _raw_argmin(hd, scales, capacity):
    buf = np.zeros(max(capacity, 1) * hd.stride, np.int32)
    n = C.c_int(-1)
    sc = np.ascontiguousarray(scales, np.float32)
    rc = hd.lib.pbd_dp_argmin(hd.h, _lib.ptr(sc, C.c_float), buf.ctypes.data, capacity, C.byref(n))
    return rc, n.value, buf.reshape(-1, hd.stride), hd.lib.pbd_last_error(hd.h).decode()


@pytest.mark.parametrize("handle", ["f32", "f64"])
def test_find_order_threshold_and_second_scan_pass(det_mod, handle):
    """One part, one mixture, 8 components, one level of 364 x 364: the root score is response + bias.  Hits at flat indices 0,
    255*4 +- 1 (a wave edge inside a block), 1023 | 1024, 2^20 - 1 | 2^20 (the scan's second pass starts there), the last one, and
    a run of 300 across a block boundary; scores equal to the threshold and NaN among them must be absent, scores one ulp above
    it present.  Count, order, (component, y, x) and the float32 score bits of every record; then a caller's capacity below the
    count, a handle's max_candidates below the count (the device stops writing), and capacity 0: the first `capacity` records
    of the same order with PBD_ERR_CAPACITY (include/pbd.h), the true count in the message."""
    R = np.float64 if handle == "f64" else np.float32
    model, resp, hits, want_rootv = _find_case(R)
    flat = model.flatten()
    HW = FIND_SIDE * FIND_SIDE
    want = [(int(i // HW), int(i % HW // FIND_SIDE), int(i % FIND_SIDE), np.float32(want_rootv[i]).view(np.uint32)) for i in hits]
    scales = np.ones(1, np.float32)
    hd = _handle(det_mod, flat, handle, max_candidates=1024)
    try:
        dp = det_mod.DynamicProgram(hd)
        _, _, _, rootv, rooti = dp.min([resp])
        assert np.array_equal(rootv[0].ravel(), want_rootv, equal_nan=True) and not rooti[0].any()
        got = dp.argmin(scales)
        assert len(got) == len(want), (len(got), len(want))
        for g, (c, y, x, sbits) in zip(got, want):
            assert (g.frame, g.level, g.component, g.root[1], g.root[0]) == (0, 0, c, y, x)
            assert np.float32(g.confidence[0]).view(np.uint32) == sbits, (c, y, x)
        rc, n, full, _ = _raw_argmin(hd, scales, 1024)
        assert rc == 0 and n == len(want)
        rc, n, rec, msg = _raw_argmin(hd, scales, 100)
        assert rc == -4 and _lib.STATUS[rc] == "PBD_ERR_CAPACITY" and n == 100 and np.array_equal(rec[:100], full[:100]), (rc, n, msg)
        assert f"{len(want)} candidates found" in msg, msg
        rc, n, rec, msg = _raw_argmin(hd, scales, 0)
        assert rc == -4 and n == 0 and not rec.any() and f"{len(want)} candidates found" in msg, (rc, n, msg)
        with pytest.raises(_lib.PbdError) as e:
            dp.argmin(scales, capacity=0)
        assert e.value.code == -4
    finally:
        hd.close()
    hd = _handle(det_mod, flat, handle, max_candidates=100)
    try:
        det_mod.DynamicProgram(hd).min([resp])
        rc, n, rec, msg = _raw_argmin(hd, scales, 1024)
        assert rc == -4 and n == 100 and np.array_equal(rec[:100], full[:100]) and not rec[100:].any(), (rc, n, msg)
        assert f"{len(want)} candidates found" in msg, msg
    finally:
        hd.close()


# ---- walk ---------------------------------------------------------------------------------------------------------------------------
def _check_argmin(det_mod, oracle, model, handle, dims, seed, max_candidates):
    """min + argmin under the half-integer scales: every record of every (level, component) against oracle.dp_argmin"""
    flat = model.flatten()
    given, ref_in = _planes(model, dims, seed, handle)
    scales = D.half_scales(len(dims))
    hd = _handle(det_mod, flat, handle, max_candidates=max_candidates)
    try:
        dp = det_mod.DynamicProgram(hd)
        dp.min(given)
        got = dp.argmin(scales)
    finally:
        hd.close()
    at = 0
    for l, s in enumerate(ref_in):
        for c in range(flat.ncomponents):
            oIx, oIy, oIk, orv, ori = oracle.dp_min(flat, c, s)
            want = oracle.dp_argmin(flat, c, l, float(scales[l]), oIx, oIy, oIk, orv, ori, capacity=orv.size + 1)
            mine = got[at:at + len(want)]
            at += len(want)
            assert len(mine) == len(want), (model.name, handle, l, c, len(mine), len(want))
            for g, w in zip(mine, want):
                where = (model.name, handle, l, dims[l], c, w["root_y"], w["root_x"])
                assert (g.level, g.component, g.root[1], g.root[0]) == (l, c, w["root_y"], w["root_x"]), where
                assert np.array_equal(g.parts, w["parts"]), where
                assert np.float32(g.confidence[0]).view(np.uint32) == np.float32(w["score"]).view(np.uint32), where
    assert at == len(got), (at, len(got))
    return len(got)


@pytest.mark.parametrize("set_name", list(D.WALK_SETS))
@pytest.mark.parametrize("handle", ["f32", "f64"])
@pytest.mark.parametrize("which", ["chain", "tree"])
def test_walk_160_parts(det_mod, oracle, which, handle, set_name):
    """kWalkMaxParts parts -- a chain of one-mixture parts, a binary tree of two-mixture parts -- with every cell a candidate and
    scales 0.5, 1.5, 2.5, 1.0, 0.75: all of k_argmin_walk's LDS rows, cvRound on exact halves (-0.5 at x == 0 among them)."""
    model = (D.chain_model if which == "chain" else D.tree_model)(160)
    dims = D.WALK_SETS[set_name]
    assert _check_argmin(det_mod, oracle, model, handle, dims, 160, 2048) == sum(h * w for h, w in dims)


def test_161_parts_are_refused(det_mod):
    rc, h, msg = _refused(det_mod, D.chain_model(161))
    assert rc == -2 and not h and "161 parts" in msg, (rc, h, msg)


@pytest.mark.parametrize("set_name", list(D.SETS))
@pytest.mark.parametrize("handle", HANDLES)
def test_ragged_model_argmin(det_mod, oracle, handle, set_name):
    """Parts of 1 to 9 mixtures in two components of different size: the walk's slot (w.slot + parent mixture) and plane
    (w.mix0 + mixture) arithmetic, a threshold that root scores hit exactly, half-integer scales."""
    n = _check_argmin(det_mod, oracle, D.ragged_model(_ksize(handle)), handle, D.SETS[set_name], D.RAGGED_SEED, 4096)
    assert n >= 300


# ---- chunked batch ----------------------------------------------------------------------------------------------------------------
def _dp_scratch_bytes(dims, JG, rs=4):
    """dp_scratch_bytes (pbd_capi.hip) of one frame whose levels are dims: cells * JG * (6 + 2 rs) + stack records * JG * 16
    (32 for double), the stack holding 64 x ceil(longest row / 2) records per wave of 64 flat rows -- or columns, if more"""
    cells = sum(h * w for h, w in dims)

    def stack(lines):       # lines: the length of every flat row (column), level after level
        return sum(64 * ((max(lines[i:i + 64]) + 1) // 2) for i in range(0, len(lines), 64))
    rows = [w for h, w in dims for _ in range(h)]
    cols = [h for h, w in dims for _ in range(w)]
    return cells * JG * (6 + 2 * rs) + max(stack(rows), stack(cols)) * JG * (16 if rs == 4 else 32)


def _chunk(per_frame, budget, want):
    while want > 1 and per_frame * want > budget:       # dp_chunk_frames
        want = (want + 1) // 2
    return want


CHUNK_FRAME = (60, 72)      # see test_chunked_batch


def test_chunked_batch(det_mod, oracle):
    """detect_batch of three equal frames with the ragged model under DP_BUDGET_MB = 1 and under the default budget, each frame
    against oracle.detect: the combine and root kernels index their scratch by the frame of the chunk (fl) and everything else by
    the frame of the batch (frame0 + fl).
    The deepest group of the model transforms 22 planes at once (depth 2: 2 + 5 + 1 + 7 mixtures in component 0, 1 + 6 in
    component 1), so a frame of C cells and S stack records needs 22 (14 C + 16 S) bytes.  dp_chunk_frames halves the chunk
    (3 -> 2 -> 1) while chunk * that exceeds the budget: 1 MB splits three frames into 2 + 1 -- the second chunk starts at
    frame0 = 2 with fl = 0, the first reaches fl = 1 -- when one frame needs more than 1/3 MB and at most 1/2 MB (more than
    1/2 MB would run them 1 + 1 + 1 and never reach fl = 1).  The arithmetic is asserted below for the frame chosen."""
    model = D.ragged_model(thresh=-1e9)
    flat = model.flatten()
    rows, cols = CHUNK_FRAME
    frames = [synth.synthetic_frame(70 + i, rows, cols, 3) for i in range(3)]
    feats, _ = oracle.features_pyramid(flat, frames[0])
    dims = [(f.shape[0], f.shape[1] // flat.flen) for f in feats]
    per_frame = _dp_scratch_bytes(dims, JG=22)
    assert (1 << 20) / 3 < per_frame <= (1 << 20) / 2, per_frame
    assert _chunk(per_frame, 1 << 20, 3) == 2 and _chunk(per_frame, 8 << 30, 3) == 3
    scores = np.sort([w["score"] for w in oracle.detect(flat, frames[0])])
    model.thresh = float(scores[-150])
    flat = model.flatten()
    want = [oracle.detect(flat, f) for f in frames]
    assert all(50 < len(w) < 2000 for w in want), [len(w) for w in want]
    for budget_mb in (1, 0):
        det = det_mod.PartsBasedDetector(device=0, max_batch=3)
        det.distributeModel(model)
        det.hd.set_debug_option(_lib.DP_BUDGET_MB, budget_mb)
        got = det.detect_batch(frames)
        det.hd.close()
        assert len(got) == sum(len(w) for w in want), (budget_mb, len(got))
        for i, w in enumerate(want):
            mine = [g for g in got if g.frame == i]
            assert len(mine) == len(w), (budget_mb, i, len(mine), len(w))
            for g, c in zip(mine, w):
                assert (g.level, g.component, g.root[1], g.root[0]) == (c["level"], c["component"], c["root_y"], c["root_x"]), (budget_mb, i)
                assert np.array_equal(g.parts, c["parts"]), (budget_mb, i)
                assert np.float32(g.score()).view(np.uint32) == np.float32(c["score"]).view(np.uint32), (budget_mb, i)
