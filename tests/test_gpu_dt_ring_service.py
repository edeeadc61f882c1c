"""The whole-wave ring service of k_dt_pass (DtRing in pbd_kernels_dp.hip) against the oracle, bit for bit, on full planes whose
neighbouring rows -- the lanes of ONE wave -- sit at different envelope depths (tests/dt_wave_replay.py: constant, pop-all ramp,
spikes, quantised, noise and staircases of 8 to 11 entries, cycling row by row and, in the transposed levels, column by column).
tests/test_dt_ring_service_cpu.py replays the service on exactly these planes and shows that they reach its events: lanes
spilling for another lane's overflow, lanes that must sit a reload out, whole-wave reloads in both halves, pop()'s own reload.

pbd_dp_min runs on fp32 and fp64 handles under the automatic launch setting, the wide ring forced (lane_shift 0) and the NARROW
ring of 16 and 32 entries (lane_shift 1, 2; cooperative kernel off), for b = -0.0 in both passes and in neither."""
import numpy as np
import pytest

from partsbaseddetector_amd import _lib

import dt_hard_planes as H
import dt_wave_replay as W

pytestmark = pytest.mark.gpu

MODELS = [("tiny", "default"), ("tiny", "linear")]
SETTINGS = {"auto": {}, "shift0": {_lib.DT_LANE_SHIFT: 0},
            "shift1/coop0": {_lib.DT_LANE_SHIFT: 1, _lib.DT_COOP: 0}, "shift2/coop0": {_lib.DT_LANE_SHIFT: 2, _lib.DT_COOP: 0}}
DEFAULTS = {_lib.DT_LANE_SHIFT: -1, _lib.DT_COOP: 1, _lib.DT_COOP_G: 0}


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


@pytest.mark.parametrize("set_name", list(W.SIZES))
@pytest.mark.parametrize("tree,deformation", MODELS)
@pytest.mark.parametrize("handle", ["f32", "f64"])
def test_dp_min_mixed_depth_planes(det_mod, oracle, handle, tree, deformation, set_name):
    flat = H.dt_model(tree, deformation).flatten()
    given = W.service_levels(flat.nfilters, set_name, 303, np.float64 if handle == "f64" else np.float32)
    bits = np.uint64 if handle == "f64" else np.uint32
    want = [[oracle.dp_min(flat, c, s) for c in range(flat.ncomponents)] for s in given]
    hd = det_mod.Handle(flat, device=0, **({"real_type": _lib.REAL_F64} if handle == "f64" else {}))
    dp = det_mod.DynamicProgram(hd)
    try:
        for setting, options in SETTINGS.items():
            for option, default in DEFAULTS.items():
                hd.set_debug_option(option, options.get(option, default))
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
