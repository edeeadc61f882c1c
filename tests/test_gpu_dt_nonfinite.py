"""pbd_dp_min on score planes that hold +-Inf and NaN, under every launch setting, against the oracle: the contract of
include/pbd.h ("Non-finite scores" at pbd_dp_min).

Class F planes (tests/dt_hard_planes.py: isolated -Inf holes, one +Inf spike, finite +-7e4 that an fp16-response handle rounds to
+-Inf) form no NaN intersection anywhere in the dynamic program -- measured: the oracle's count is 0 -- and every output must
equal the reference's bit for bit.  Class N planes (a masked region with a whole row and column of -Inf, neighbouring +Inf, NaN
cells) do form some -- measured: the count is above 0 -- and every output must equal the oracle run with the "max" read-out,
max{k : z[k] < os + q} with comparisons against NaN false, whichever kernel variant the launch picks: the streamed ring kernels
walk down from the top, the cooperative kernel searches z[] and walks down instead in rows that pushed a NaN.  rootv is compared
as "NaN at the same places, the same bits elsewhere" (the default NaN of a CPU and of the GPU differ in sign and payload); the
integer planes byte for byte, whole planes.  test_inputs_reach_the_paths replays the leaf parts' planes to show that class N rows
do pass through ring spill and reload, with a NaN entry among the spilled, and do pop a whole cooperative window."""
import functools

import numpy as np
import pytest

from partsbaseddetector_amd import _lib
from partsbaseddetector_amd import synth

import dt_hard_planes as H
from test_gpu_dt_planes import HANDLES, SETTINGS, _force, _handle, _paths

pytestmark = pytest.mark.gpu

# (rows, cols, base kind: every one exact in fp16).  u8: the edges of the 16-element chunk and of the 8- and 16-lane cooperative
# windows; constant planes keep every element on the envelope (depth = line length), plateaus with spikes give long pop runs.
# i16 (a side above 256: int16 position planes for the whole launch, never cooperative): the last two levels' rows and columns of
# 530 constant elements are deeper than the deepest ring (8 << 6 = 512 entries).
LEVELS = {
    "u8": [(16, 65, "spikes"), (33, 33, "quantised"), (17, 128, "constant"), (3, 17, "quantised"), (2, 2, "quantised"),
           (1, 1, "quantised"), (31, 64, "spikes")],
    "i16": [(3, 300, "constant"), (257, 2, "constant"), (2, 530, "constant"), (530, 2, "constant")],
}
MODELS = [("tiny", "default"), ("tree", "xlinear"), ("tree", "pow2_linear")]
KINDS = H.NONFINITE_F + H.NONFINITE_N


def _readout(kind):
    return "max" if kind in H.NONFINITE_N else "reference"


@functools.lru_cache(maxsize=None)
def _flat(tree, deformation):
    return H.dt_model(tree, deformation).flatten()


@functools.lru_cache(maxsize=None)
def _inputs(handle, tree, deformation, kind, set_name):
    """The score planes of one case: what the handle is given and what the oracle must be run on (an fp16-response handle rounds
    its input to fp16; only f16_sat changes under that rounding)."""
    flat = _flat(tree, deformation)
    seed = 1000 * KINDS.index(kind) + {"u8": 11, "i16": 22}[set_name]
    given = H.nonfinite_scores(flat, kind, LEVELS[set_name], seed, np.float64 if handle == "f64" else np.float32)
    if handle != "f16":
        return given, given
    with np.errstate(over="ignore"):
        rounded = [g.astype(np.float16).astype(np.float32) for g in given]
    if kind == "f16_sat":
        assert all(np.isfinite(g).all() for g in given) and any(np.isinf(r).any() for r in rounded)
    else:
        assert all(np.array_equal(g, r, equal_nan=True) for g, r in zip(given, rounded))
    return given, rounded


@functools.lru_cache(maxsize=None)
def _want(oracle, handle, tree, deformation, kind, set_name):
    """The oracle's dp_min of every (level, component) under the kind's read-out, and its NaN intersections per call."""
    flat = _flat(tree, deformation)
    want, nans = [], []
    for s in _inputs(handle, tree, deformation, kind, set_name)[1]:
        per = []
        for c in range(flat.ncomponents):
            per.append(oracle.dp_min(flat, c, s, readout=_readout(kind)))
            nans.append(oracle.nan_isect())
        want.append(per)
    return want, nans


def _applies(handle, kind):
    return kind != "f16_sat" or handle == "f16"      # finite +-7e4 are ordinary scores to the other handles


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.fixture(scope="module")
def handles(det_mod):
    """One handle per (handle kind, model), shared by the settings; closed when the module is done."""
    cache = {}

    def get(handle, tree, deformation):
        key = (handle, tree, deformation)
        if key not in cache:
            cache[key] = _handle(det_mod, _flat(tree, deformation), handle)
        return cache[key]
    yield get
    for hd in cache.values():
        hd.close()


def _same_reals(got, want, bits):
    """NaN at the same places, the same bits everywhere else."""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got[~gn].view(bits), want[~wn].view(bits))


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("tree,deformation", MODELS)
@pytest.mark.parametrize("handle", HANDLES)
def test_dp_min_nonfinite(det_mod, handles, oracle, handle, tree, deformation, setting):
    flat = _flat(tree, deformation)
    bits = np.uint64 if handle == "f64" else np.uint32
    hd = handles(handle, tree, deformation)
    dp = det_mod.DynamicProgram(hd)
    _force(hd, SETTINGS[setting])
    try:
        for kind in KINDS:
            if not _applies(handle, kind):
                continue
            for set_name in LEVELS:
                given, _ = _inputs(handle, tree, deformation, kind, set_name)
                want, nans = _want(oracle, handle, tree, deformation, kind, set_name)
                if kind in H.NONFINITE_F:
                    assert max(nans) == 0, (kind, set_name, nans)       # membership is measured: no NaN intersection at all
                else:
                    assert sum(nans) > 0, (kind, set_name, nans)
                Ix, Iy, Ik, rootv, rooti = dp.min(given)
                for l in range(len(given)):
                    for c in range(flat.ncomponents):
                        oIx, oIy, oIk, orv, ori = want[l][c]
                        where = (kind, set_name, l, given[l].shape[1:], c)
                        assert _same_reals(rootv[l][c], orv, bits), where
                        assert np.array_equal(rooti[l][c], ori), where
                        p0, p1 = flat.part_offset[c], flat.part_offset[c + 1]
                        for gp in range(p0 + 1, p1):
                            par = p0 + flat.parentid[gp]
                            for m in range(flat.mix_offset[par + 1] - flat.mix_offset[par]):
                                sl = flat.ptr_slot[gp] + m
                                assert np.array_equal(Ik[l][sl], oIk[sl]), where + (gp, m, "Ik")
                                assert np.array_equal(Ix[l][sl], oIx[sl]), where + (gp, m, "Ix")
                                assert np.array_equal(Iy[l][sl], oIy[sl]), where + (gp, m, "Iy")
    finally:
        _force(hd, {})


@pytest.mark.parametrize("handle", HANDLES)
def test_inputs_reach_the_paths(handle):
    """computeRow replayed on the leaf parts' class N planes (their transforms' input is the raw plane): for each forced setting,
    some row that pushed a NaN intersection is so deep that its lowest NaN entry lies more than that setting's ring below its
    top -- the entry is spilled, and reloaded with the intersection recomputed on NaN operands -- and, where the setting runs
    the cooperative kernel, some such row pops a whole window for one element."""
    R = np.float64 if handle == "f64" else np.float32
    stats = {}      # (set, pass) -> most entries between the top and the lowest NaN entry, most pops, over rows with a NaN intersection
    for tree, deformation in MODELS:
        flat = _flat(tree, deformation)
        for set_name in LEVELS:
            for kind in H.NONFINITE_N:
                for s in _inputs(handle, tree, deformation, kind, set_name)[1]:
                    for f, ax, bx, ay, by, osx, osy in H.leaf_jobs(flat):
                        _, st_r, st_c = H.replay_dt(s[f], ax, bx, ay, by, osx, osy, R, readout="max")
                        for pas, st in (("rows", st_r), ("cols", st_c)):
                            n = st["nan_isect"] > 0
                            if n.any():
                                d, p = stats.get((set_name, pas), (0, 0))
                                stats[(set_name, pas)] = (max(d, int((st["top"] + 1 - st["nan_floor"])[n].max())),
                                                          max(p, int(st["maxpop"][n].max())))
    for setting, options in SETTINGS.items():
        if not options:
            continue
        reached = {}
        for set_name in LEVELS:
            for pas, (form, size) in _paths(handle, options, set_name).items():
                d, p = stats.get((set_name, pas), (0, 0))
                got = d >= size + 2 if form == "ring" else p >= size     # a ring of T spills once T + 2 entries are live
                reached[(form, size)] = reached.get((form, size), False) or got
        assert all(reached.values()), (setting, reached, stats)


# ---- the detect path on fp16 responses that saturate ------------------------------------------------------------------------
def saturating_model(thresh):
    """The pow2 tree with a bank, set through Model.from_vector, whose weights sit on the truncation channel alone: that feature
    is 0 inside a level and 1 in its constant border, so a response is the sum of the taps that fall outside -- exact in fp16
    operands and fp32 accumulation, whatever the image holds, and the handle's fp16 response is that sum rounded once.  Every
    filter has taps of multiples of 1/8; ten of the fifteen also have three taps of -3e4 which all fall outside at the bottom
    left cell only: -9e4 there, -Inf as fp16, -6e4 (finite) along the left and bottom edges."""
    from partsbaseddetector_amd.examples import vector_offsets
    base = H.dt_model("tree", "pow2")
    flat = base.flatten()
    w = base.to_vector()
    _, fbase, _ = vector_offsets(flat)
    rng = np.random.default_rng(17)
    w[fbase:] = 0
    for f in range(flat.nfilters):
        k = int(flat.filter_ksize[f])
        filt = np.zeros((k, k, flat.flen), np.float32)
        filt[:, :, flat.flen - 1] = rng.integers(-8, 9, (k, k)) * 0.125
        if f % 3 != 1:
            for i, j in ((1, 1), (3, 3), (3, 1)):
                filt[i, j, flat.flen - 1] = -3e4
        o = fbase + int(flat.filter_offset[f])
        w[o:o + filt.size] = filt.ravel()
    model = base.from_vector(w)
    model.thresh = thresh
    return model


def _detect_on_fp16_responses(oracle, flat, im):
    """The oracle's detect with its responses rounded to fp16, as the handle keeps them: features, responses, rounding, dp_min
    and argmin per (level, component) -- detect's own order.  Also the infinite responses, whether two of them are neighbours in
    a plane, and the NaN intersections of all the dp_min calls."""
    feats, scales = oracle.features_pyramid(flat, im)
    cands, ninf, neighbours, nans = [], 0, False, 0
    for l, ft in enumerate(feats):
        with np.errstate(over="ignore"):
            r16 = oracle.responses(flat, ft).astype(np.float16).astype(np.float32)
        inf = np.isinf(r16)
        ninf += int(inf.sum())
        neighbours |= bool((inf[:, 1:, :] & inf[:, :-1, :]).any() or (inf[:, :, 1:] & inf[:, :, :-1]).any())
        for c in range(flat.ncomponents):
            Ix, Iy, Ik, rootv, rooti = oracle.dp_min(flat, c, r16)
            nans += oracle.nan_isect()
            cands += oracle.dp_argmin(flat, c, l, scales[l], Ix, Iy, Ik, rootv, rooti)
    return cands, ninf, neighbours, nans


def test_detect_batch_on_saturated_fp16_responses(det_mod, oracle):
    """detect_batch on an fp16-response handle whose bank drives a few responses of every level past fp16's range.  On the CPU:
    the rounded responses hold isolated infinities and no NaN intersection forms (class F).  The candidates equal the oracle's
    detect on those responses under the default launch, the cooperative kernel forced and the narrow ring forced.  (The responses
    do not depend on the image: what this case adds to pbd_dp_min's is the detect path -- resident fp16 responses, the batched
    passes, find and walk -- on infinite scores.)"""
    model = saturating_model(thresh=10.5)
    flat = model.flatten()
    frames = [synth.synthetic_frame(60 + i, 70, 150, 3) for i in range(2)]
    want = []
    for f in frames:
        cands, ninf, neighbours, nans = _detect_on_fp16_responses(oracle, flat, f)
        assert ninf >= 10 and not neighbours and nans == 0, (ninf, neighbours, nans)
        assert 20 < len(cands) < 2000, len(cands)
        want.append(cands)
    for setting in ("auto", "shift3", "shift3/coop0"):
        det = det_mod.PartsBasedDetector(device=0, conv_mode=_lib.CONV_MFMA_F16, max_batch=2)
        det.distributeModel(model)
        _force(det.hd, SETTINGS[setting])
        got = det.detect_batch(frames)
        try:
            assert len(got) == sum(len(w) for w in want), (setting, len(got))
            for i, w in enumerate(want):
                mine = [g for g in got if g.frame == i]
                assert len(mine) == len(w), (setting, i, len(mine), len(w))
                for g, c in zip(mine, w):
                    assert (g.level, g.component, g.root[1], g.root[0]) == (c["level"], c["component"], c["root_y"], c["root_x"]), (setting, i)
                    assert np.array_equal(g.parts, c["parts"]), (setting, i)
                    assert np.float32(g.score()).view(np.uint32) == np.float32(c["score"]).view(np.uint32), (setting, i)
        finally:
            det.hd.close()
