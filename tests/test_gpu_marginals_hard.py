"""pbd_max_marginals, pbd_get_marginals and pbd_marginal_poses on the hard cases of tests/marginal_cases.py, against the numpy rule of
partsbaseddetector_amd/marginals.py (tests/test_marginals_hard_cpu.py checks the cases and the rule on the CPU):

* the wide models ("wide8", "wide16": the 8- and 16-type instantiations of k_mm_messages, reductions over up to 16 parent types,
  Jk of 8 and above with ties among them, slices that resume every parent type and every four), every plane byte for byte and the
  decoded poses word for word;
* responses with +-Inf and NaN cells under every distance-transform launch setting Handle.set_debug_option can force: the yardstick
  is the rule run with the "max" read-out (include/pbd.h, pbd_dp_min, "Non-finite scores", item 3; the mirrored transforms follow
  it as the upward ones do).  mm and down are compared as "NaN at the same places, the same bits elsewhere" (the sign and payload
  of a NaN are unspecified), Jx / Jy / Jk as whole integer planes.  No comparison is left out because the yardstick holds a NaN.
  Every kind runs on both level sets under every setting: the yardsticks are computed once per (handle, model, kind, level set)
  and shared by the settings, so the first (setting, model, handle, level set) to need them takes up to two seconds ("wide16" on
  "i16") and the others well under one;
* the poses decoded from such planes -- every part's best finite cell, cells where every mm of the part is NaN or -Inf with type
  -1 (type 0, whose mm is the score), bad seeds -- under the default launch and a forced narrow ring;
* the finite dyadic cases "tree", "slices" and "wide16" on level set B under every forced setting, byte for byte."""
import numpy as np
import pytest

import marginal_cases as MC
from partsbaseddetector_amd import _lib, detector
from test_gpu_dt_planes import SETTINGS, _force
from test_gpu_dt_nonfinite import _same_reals

pytestmark = pytest.mark.gpu

REAL = {"f32": (_lib.REAL_F32, "float32", np.uint32), "f64": (_lib.REAL_F64, "float64", np.uint64)}
HANDLES = tuple(REAL)
SENT = -7
WHAT = (("mm", _lib.MM_VALUES), ("down", _lib.MM_DOWN), ("Jx", _lib.MM_PARENT_X), ("Jy", _lib.MM_PARENT_Y), ("Jk", _lib.MM_PARENT_K))
FINITE_CASES = [("tree", "B"), ("slices", "B"), ("wide16", "B")]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def handles():
    """One handle per (handle kind, model, value set), shared by the settings; closed when the module is done."""
    cache = {}

    def get(handle, name, values):
        key = (handle, name, values)
        if key not in cache:
            cache[key] = detector.Handle(MC.model(name, values), device=0, max_candidates=1 << 12, real_type=REAL[handle][0])
        return cache[key]
    yield get
    for hd in cache.values():
        hd.close()


def _check_bytes(hd, shapes, want_of, where):
    for key, what in WHAT:
        want = want_of(key)
        for l, (H, W) in enumerate(shapes):
            got = hd.get_marginals(l, what, H, W)
            assert got.dtype == want[l].dtype and got.shape == want[l].shape, where + (key, l)
            assert got.tobytes() == want[l].tobytes(), where + (key, l, np.argwhere(got != want[l])[:4])


def _check_nonfinite(hd, shapes, ys, bits, where):
    for key, what in WHAT:
        for l, (H, W) in enumerate(shapes):
            got, want = hd.get_marginals(l, what, H, W), ys[l][0][key]
            assert got.dtype == want.dtype and got.shape == want.shape, where + (key, l)
            if key in ("mm", "down"):
                assert _same_reals(got, want, bits), where + (key, l, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
            else:
                assert np.array_equal(got, want), where + (key, l, np.argwhere(got != want)[:4])


def _check_poses(got, want, where):
    """status, records and placements; the score word with every NaN made the same one"""
    got, want = [np.array(a, copy=True) for a in got], [np.array(a, copy=True) for a in want]
    for a in (got[1], want[1]):
        ok = got[0] > 0
        sc = a[ok, 5].view(np.float32)
        sc[np.isnan(sc)] = np.nan
        a[ok, 5] = sc.view(np.int32)
    for g, w, what in zip(got, want, ("status", "records", "place")):
        assert np.array_equal(g, w), where + (what, np.argwhere(g != w)[:4])


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("values", MC.VALUES)
@pytest.mark.parametrize("name,levels", MC.WIDE_CASES)
def test_wide_models_every_plane_and_pose(handles, name, levels, values, handle):
    dtype = REAL[handle][1]
    hd = handles(handle, name, values)
    detector.DynamicProgram(hd).min(MC.responses(name, levels, values, dtype))
    hd.max_marginals(0)
    _check_bytes(hd, MC.LEVEL_SETS[levels], lambda key: MC.merged(name, levels, values, dtype, key), (name, levels, values))
    seeds = MC.seeds_of(name, levels, values, dtype)
    want = MC.decode_all(name, levels, values, dtype, seeds, frame_offset=5, fill=SENT)
    assert (want[0] > 0).sum() >= 6 and (want[0] == -1).sum() == 9
    got = hd.marginal_poses(seeds, MC.scales(levels), 5, fill=SENT)
    for g, w, what in zip(got, want, ("status", "records", "place")):
        assert np.array_equal(g, w), (what, np.argwhere(g != w)[:4])


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("set_name", MC.NF_SETS)
@pytest.mark.parametrize("name", [m for m, _ in MC.NF_MODELS])
@pytest.mark.parametrize("handle", HANDLES)
def test_nonfinite_marginals_every_setting(handles, handle, name, set_name, setting):
    _, dtype, bits = REAL[handle]
    hd = handles(handle, name, MC.nf_values(name))
    dp = detector.DynamicProgram(hd)
    _force(hd, SETTINGS[setting])
    try:
        for kind in MC.NF_KINDS:
            ys, _ = MC.nf_yardstick(name, kind, set_name, dtype)
            dp.min(MC.nf_responses(name, kind, set_name, dtype))
            hd.max_marginals(0)
            _check_nonfinite(hd, MC.nf_shapes(set_name), ys, bits, (kind,))
    finally:
        _force(hd, {})


@pytest.mark.parametrize("setting", ["auto", "shift3/coop0"])
@pytest.mark.parametrize("name", [m for m, _ in MC.NF_MODELS])
@pytest.mark.parametrize("handle", HANDLES)
def test_nonfinite_poses(handles, handle, name, setting):
    _, dtype, _ = REAL[handle]
    flat = MC.model(name, MC.nf_values(name)).flatten()
    hd = handles(handle, name, MC.nf_values(name))
    dp = detector.DynamicProgram(hd)
    _force(hd, SETTINGS[setting])
    try:
        decoded = nan_seeds = neginf_seeds = 0
        for kind in MC.NF_KINDS:
            for set_name in MC.NF_SETS:
                ys, _ = MC.nf_yardstick(name, kind, set_name, dtype)
                cells = MC.nf_cells(name, kind, set_name, dtype)
                seeds = MC.nf_seeds(name, kind, set_name, dtype)
                sc = MC.nf_scales(set_name)
                want = MC.decode_seeds(flat, ys, MC.nf_shapes(set_name), sc, dtype, seeds, 3, SENT)
                assert (want[0] == -1).sum() == 9
                dp.min(MC.nf_responses(name, kind, set_name, dtype))
                hd.max_marginals(0)
                _check_poses(hd.marginal_poses(seeds, sc, 3, fill=SENT), want, (kind, set_name))
                decoded += int((want[0] > 0).sum())
                nan_seeds += len(cells["nan"])
                neginf_seeds += len(cells["neginf"])
        assert decoded > 40 and nan_seeds > 0 and neginf_seeds > 0
    finally:
        _force(hd, {})


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "auto"])
@pytest.mark.parametrize("name,levels", FINITE_CASES)
@pytest.mark.parametrize("handle", HANDLES)
def test_finite_cases_every_setting(handles, handle, name, levels, setting):
    dtype = REAL[handle][1]
    hd = handles(handle, name, "dyadic")
    _force(hd, SETTINGS[setting])
    try:
        detector.DynamicProgram(hd).min(MC.responses(name, levels, "dyadic", dtype))
        hd.max_marginals(0)
        _check_bytes(hd, MC.LEVEL_SETS[levels], lambda key: MC.merged(name, levels, "dyadic", dtype, key), (name, levels))
    finally:
        _force(hd, {})
