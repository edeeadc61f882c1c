"""Every distance-transform kernel variant (k_dt_pass for rows and columns, k_dt_coop in pbd_kernels_dp.hip) against the oracle, bit for
bit, on full planes of hard inputs.

pbd_dp_min runs under each launch setting Handle.set_debug_option can force -- rows per wave (lane_shift 0..6: wide ring,
NARROW ring of 8 << lane_shift entries), the cooperative kernel on or off, 4 or 8 rows per cooperative wave -- on fp32, fp64 and
fp16-response handles, for small trees whose deformations give b = -0.0 in both passes, in neither, in the columns pass only,
and power-of-two quadratics (exact intersection arithmetic, hence exact ties).  The levels sit at the edges of the 16-element
chunk, the 8- and 16-lane cooperative windows and the uint8 position planes; the planes (tests/dt_hard_planes.py) are constant
(envelopes as deep as the row: ring spill and reload), smooth, plateaus with spikes (long pop runs: the cooperative kernel's
lower block, chains of reloads), quantised (exact ties in the pop test and in the read-out) and of wide dynamic range.
test_inputs_reach_the_paths replays computeRow on the leaf parts' planes to show that the inputs do reach those paths."""
import numpy as np
import pytest

from partsbaseddetector_amd import _lib
from partsbaseddetector_amd import synth

import dt_hard_planes as H

pytestmark = pytest.mark.gpu

# (rows, cols, plane kind or None: rotating through every kind).  U8: no side above 256 (uint8 position planes, the cooperative
# kernel can run); flat rows 701 and columns 1025, multiples of neither 4, 8 nor 64 >> lane_shift for lane_shift < 6
SETS = {
    "u8": [(1, 256, None), (256, 1, "constant"), (2, 255, None), (255, 3, None), (15, 129, None), (17, 128, "constant"),
           (16, 65, "spikes"), (31, 64, None), (33, 33, "quantised"), (3, 17, None), (2, 2, None), (1, 1, None), (4, 7, None),
           (65, 64, None)],
    # sides above 256: int16 planes for the whole launch, never cooperative; rows of 600 constant elements are deeper than the
    # NARROW ring of one lane (8 << 6 = 512 entries); flat rows 875, columns 1195
    "i16": [(3, 600, "constant"), (600, 3, "constant"), (2, 257, None), (257, 2, "spikes"), (5, 300, "quantised"),
            (8, 33, None)],
}
MODELS = [("tiny", "default"), ("tiny", "linear"), ("tree", "xlinear"), ("tree", "pow2"), ("tree", "pow2_linear")]
HANDLES = ("f32", "f64", "f16")

SETTINGS = {"auto": {}}
SETTINGS.update({f"shift{s}": {_lib.DT_LANE_SHIFT: s} for s in range(7)})
SETTINGS.update({f"shift{s}/coop0": {_lib.DT_LANE_SHIFT: s, _lib.DT_COOP: 0} for s in (3, 4, 6)})
SETTINGS.update({f"shift{s}/g{g}": {_lib.DT_LANE_SHIFT: s, _lib.DT_COOP_G: g} for s in (3, 4) for g in (4, 8)})
DEFAULTS = {_lib.DT_LANE_SHIFT: -1, _lib.DT_COOP: 1, _lib.DT_COOP_G: 0}


def _inputs(handle, flat, set_name):
    """The score planes of one (handle, model, set): what the handle is given and what the oracle must be run on."""
    seed = {"u8": 101, "i16": 202}[set_name]
    if handle == "f16":
        # fp16 responses: the wide planes keep to fp16's range (scores that saturate to +-Inf, and infinite and NaN scores on
        # every handle: tests/test_gpu_dt_nonfinite.py)
        given = H.level_scores(flat.nfilters, SETS[set_name], seed, np.float32, big=3e4)
        return given, [g.astype(np.float16).astype(np.float32) for g in given]
    given = H.level_scores(flat.nfilters, SETS[set_name], seed, np.float64 if handle == "f64" else np.float32)
    return given, given


def _handle(det_mod, flat, handle):
    kw = {"f32": {}, "f64": {"real_type": _lib.REAL_F64}, "f16": {"conv_mode": _lib.CONV_MFMA_F16}}[handle]
    return det_mod.Handle(flat, device=0, **kw)


def _force(hd, options):
    for option, default in DEFAULTS.items():
        hd.set_debug_option(option, options.get(option, default))


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.mark.parametrize("set_name", list(SETS))
@pytest.mark.parametrize("tree,deformation", MODELS)
@pytest.mark.parametrize("handle", HANDLES)
def test_dp_min_planes_every_setting(det_mod, oracle, handle, tree, deformation, set_name):
    flat = H.dt_model(tree, deformation).flatten()
    given, ref_in = _inputs(handle, flat, set_name)
    bits = np.uint64 if handle == "f64" else np.uint32
    want = [[oracle.dp_min(flat, c, s) for c in range(flat.ncomponents)] for s in ref_in]
    hd = _handle(det_mod, flat, handle)
    dp = det_mod.DynamicProgram(hd)
    try:
        for setting, options in SETTINGS.items():
            _force(hd, options)
            Ix, Iy, Ik, rootv, rooti = dp.min(given)
            for l in range(len(given)):
                for c in range(flat.ncomponents):
                    oIx, oIy, oIk, orv, ori = want[l][c]
                    where = (setting, l, given[l].shape[1:], c)
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
    finally:
        hd.close()


def _paths(handle, options, set_name):
    """The form each pass of a forced setting runs on a set: ("ring", entries per lane) or ("coop", window) -- the launchers'
    choice (launch_dt_rows / launch_dt_cols / launch_dt_coop)."""
    sh = options[_lib.DT_LANE_SHIFT]
    coop = options.get(_lib.DT_COOP, 1) and sh >= 3 and set_name == "u8" and handle != "f64"
    window = 8 if options.get(_lib.DT_COOP_G, 0) == 8 else 16
    ring = ("ring", 8 << sh if sh > 0 else 8)
    rows = ("ring", 8) if handle == "f16" else (("coop", window) if coop else ring)     # fp16 rows: the wide ring only
    cols = ("coop", window) if coop else ring
    return {"rows": rows, "cols": cols}


@pytest.mark.parametrize("handle", HANDLES)
def test_inputs_reach_the_paths(handle):
    """computeRow replayed on the leaf parts' planes (their transforms' input is the raw plane) of every model and set: for each
    forced setting, some rows it runs through a ring are deeper than that ring (spill and reload), some rows it runs through the
    cooperative kernel pop a whole window for one element (the lower-block fetch), and every set has exact ties s == z[k] in the
    pop test and z[k+1] == os in the read-out, in both passes."""
    R = np.float64 if handle == "f64" else np.float32
    stats = {}      # (set, pass) -> max depth, max pops, scan tie, read-out tie
    for tree, deformation in MODELS:
        flat = H.dt_model(tree, deformation).flatten()
        for set_name in SETS:
            _, ref_in = _inputs(handle, flat, set_name)
            for f, ax, bx, ay, by, osx, osy in H.leaf_jobs(flat):
                for s in ref_in:
                    _, st_r, st_c = H.replay_dt(s[f], ax, bx, ay, by, osx, osy, R)
                    for pas, st in (("rows", st_r), ("cols", st_c)):
                        d, p, ts, tr = stats.get((set_name, pas), (0, 0, False, False))
                        stats[(set_name, pas)] = (max(d, int(st["depth"].max())), max(p, int(st["maxpop"].max())),
                                                  ts or bool(st["scan_tie"].any()), tr or bool(st["read_tie"].any()))
    for key, (_, _, ts, tr) in stats.items():
        assert ts and tr, (key, stats[key])
    for setting, options in SETTINGS.items():
        if not options:
            continue
        reached = {}
        for set_name in SETS:
            for pas, (form, size) in _paths(handle, options, set_name).items():
                d, p, _, _ = stats[(set_name, pas)]
                got = d >= size + 2 if form == "ring" else p >= size     # a ring of T spills once T + 2 entries are live
                reached[(form, size)] = reached.get((form, size), False) or got
        assert all(reached.values()), (setting, reached, stats)


def test_detect_batch_every_setting(det_mod, oracle):
    """detect_batch on three frames of one size under every forced setting equals the oracle's detect of each frame, in order:
    the frame index of the batched passes (frame0, blockIdx.y), which pbd_dp_min's single frame never uses."""
    model = H.dt_model("tree", "pow2", thresh=2.25)
    flat = model.flatten()
    frames = [synth.synthetic_frame(60 + i, 110, 270, 3) for i in range(3)]
    want = [oracle.detect(flat, f) for f in frames]
    assert all(20 < len(w) < 2000 for w in want), [len(w) for w in want]
    for setting, options in SETTINGS.items():
        det = det_mod.PartsBasedDetector(device=0, max_batch=3)
        det.distributeModel(model)
        _force(det.hd, options)
        got = det.detect_batch(frames)
        assert len(got) == sum(len(w) for w in want), (setting, len(got))
        for i, w in enumerate(want):
            mine = [g for g in got if g.frame == i]
            assert len(mine) == len(w), (setting, i, len(mine), len(w))
            for g, c in zip(mine, w):
                assert (g.level, g.component, g.root[1], g.root[0]) == (c["level"], c["component"], c["root_y"], c["root_x"]), (setting, i)
                assert np.array_equal(g.parts, c["parts"]), (setting, i)
                assert np.float32(g.score()).view(np.uint32) == np.float32(c["score"]).view(np.uint32), (setting, i)
        det.hd.close()
