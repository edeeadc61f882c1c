"""pbd_cluster_parts and pbd_cluster_parts_device against their yardstick cluster_parts_ref (partsbaseddetector_amd/trainmodel.py),
bit for bit on every output, on the built cases of tests/cluster_cases.py and on the smallest shapes at which the kernels can go
wrong: point counts around a lane, a wave and the 1024-lane stride, K = 1, 2, 6 and 16 mixed in one call (both register variants
of k_km_trials), one trial and a hundred, more (part, trial) pairs than the grid holds, trials cut off by max_iter while labels
still change, a handle reused at other sizes, and every refused argument."""

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import trainmodel as TM

import cluster_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def hd():
    h = detector.Handle(M.synthetic_tiny_model())
    yield h
    h.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_doubles(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got[ok]), bits(want[ok])), (what, got[ok][bits(got[ok]) != bits(want[ok])][:4])


def same(got, want, all_trials=True):
    assert np.array_equal(got["idx"], want["idx"])
    same_doubles(got["centres"], want["centres"], "centres")
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["anchors"], want["anchors"])
    assert np.array_equal(got["info"]["best_trial"], want["info"]["best_trial"])
    assert np.array_equal(got["info"]["iterations"], want["info"]["iterations"])
    same_doubles(got["info"]["sumdist"], want["info"]["sumdist"], "info.sumdist")
    if all_trials:
        same_doubles(got["sumdist_all"], want["sumdist_all"], "sumdist_all")
        assert np.array_equal(got["iters_all"], want["iters_all"])


def run_device(hd, d, parent, K, kw, want_all=True):
    """pbd_cluster_parts_device on torch buffers -> the host form's dict"""
    import torch
    P, N, T = d.shape[0], d.shape[1], kw["trials"]
    t_def = torch.from_numpy(np.array(d, np.float64)).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    idx, cen, cnt, anc = z((P, N), torch.int32), z((P, 16, 2), torch.float64), z((P, 16), torch.int32), z((P, 16, 2), torch.int32)
    info, sd, its = z((P, 16), torch.uint8), z((P, T), torch.float64), z((P, T), torch.int32)
    torch.cuda.synchronize()
    hd.cluster_parts_device(P, N, t_def.data_ptr(), parent, K, T, kw["max_iter"], kw["seed"], idx.data_ptr(), cen.data_ptr(),
                            cnt.data_ptr(), anc.data_ptr(), info.data_ptr(), sd.data_ptr() if want_all else None,
                            its.data_ptr() if want_all else None)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    out = {"idx": idx.cpu().numpy(), "centres": cen.cpu().numpy(), "counts": cnt.cpu().numpy(), "anchors": anc.cpu().numpy(),
           "info": info.cpu().numpy().reshape(-1).view(_lib.CLUSTER_INFO_DTYPE), "sumdist_all": sd.cpu().numpy(),
           "iters_all": its.cpu().numpy()}
    if not want_all:
        assert not out["sumdist_all"].any() and not out["iters_all"].any()
    return out


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_built_cases_host_and_device(hd, name):
    d, parent, K, kw, want = CC.case(name)
    same(hd.cluster_parts(d, parent, K, **kw), want)
    same(run_device(hd, d, parent, K, kw), want)


@pytest.mark.parametrize("npos", CC.SHAPE_NPOS)
def test_point_counts_around_lane_wave_and_stride(hd, npos):
    d, parent, K, kw, want = CC.case((npos,))
    assert sorted(K) == [1, 2, 6, 16]
    same(hd.cluster_parts(d, parent, K, **kw), want)


def test_one_trial_and_no_per_trial_outputs(hd):
    d, parent, K, kw, want = CC.case((65, 1))
    assert kw["trials"] == 1
    same(hd.cluster_parts(d, parent, K, **kw), want)
    same(hd.cluster_parts(d, parent, K, want_all=False, **kw), want, all_trials=False)
    same(run_device(hd, d, parent, K, kw, want_all=False), want, all_trials=False)


def test_more_pairs_than_the_grid(hd):
    d, parent, K, kw = CC.shape(65)
    d, parent, K, kw = d[:2], parent[:2], [2, 3], dict(kw, trials=_lib.KM_MAX_GRID // 2 + 40)
    assert len(K) * kw["trials"] > _lib.KM_MAX_GRID
    want = TM.cluster_parts_ref(d, parent, K, **kw)
    same(hd.cluster_parts(d, parent, K, **kw), want)
    beyond = want["sumdist_all"].ravel()[_lib.KM_MAX_GRID:]        # the pairs a workgroup takes on its second round
    assert len(beyond) >= 64 and len(set(beyond.tolist())) > 1


@pytest.mark.parametrize("cut", [1, 2])
def test_max_iter_cuts_trials_off(hd, cut):
    d, parent, K, kw, full = CC.case((1025,))
    d, parent, K, kw, want = CC.case((1025, 3, cut))
    assert np.any(full["iters_all"] > cut) and want["iters_all"].max() == cut
    same(hd.cluster_parts(d, parent, K, **kw), want)


def test_workspace_reuse_across_sizes(hd):
    for key in ((2500,), (63,), "grid", (2500,), (1,)):
        d, parent, K, kw, want = CC.case(key)
        same(hd.cluster_parts(d, parent, K, **kw), want)


def test_double_handle_gives_the_same(hd):
    h64 = detector.Handle(M.synthetic_tiny_model(), real_type=_lib.REAL_F64)
    try:
        for key in ("order257", (1025,)):
            d, parent, K, kw, want = CC.case(key)
            same(h64.cluster_parts(d, parent, K, **kw), want)
    finally:
        h64.close()


def test_detector_method(hd):
    det = detector.PartsBasedDetector()
    det.distributeModel(M.synthetic_tiny_model())
    try:
        d, parent, K, kw, want = CC.case("tree")
        same(det.clusterParts(d, parent, K, **kw), want)
    finally:
        det.hd.close()


@pytest.mark.parametrize("bad", [
    dict(nparts=1), dict(npos=0), dict(trials=0), dict(max_iter=0), dict(K=[0, 2]), dict(K=[2, 17]), dict(parent=[0, 0]),
    dict(parent=[-1, 1]), dict(parent=[-1, -1]), dict(trials=(1 << 19) + 1), dict(null="def"), dict(null="idx")])
def test_invalid_arguments_are_refused(hd, bad):
    import torch
    kw = dict(nparts=2, npos=4, trials=2, max_iter=5, K=[2, 2], parent=[-1, 0], null=None)
    kw.update(bad)
    d = np.zeros((2, 4, 2))
    pa, K = np.array(kw["parent"], np.int32), np.array(kw["K"], np.int32)
    idx, cen, cnt, anc = np.zeros((2, 4), np.int32), np.zeros((2, 16, 2)), np.zeros((2, 16), np.int32), np.zeros((2, 16, 2), np.int32)
    info = np.zeros(2, _lib.CLUSTER_INFO_DTYPE)
    p = lambda a, name: None if kw["null"] == name else a.ctypes.data
    rc = hd.lib.pbd_cluster_parts(hd.h, kw["nparts"], kw["npos"], p(d, "def"), pa.ctypes.data, K.ctypes.data, kw["trials"],
                                  kw["max_iter"], 0, p(idx, "idx"), cen.ctypes.data, cnt.ctypes.data, anc.ctypes.data,
                                  info.ctypes.data, None, None)
    assert rc == -1
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    q = lambda name: None if kw["null"] == name else t.data_ptr()
    rc = hd.lib.pbd_cluster_parts_device(hd.h, kw["nparts"], kw["npos"], q("def"), pa.ctypes.data, K.ctypes.data, kw["trials"],
                                         kw["max_iter"], 0, q("idx"), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None)
    assert rc == -1
    # the handle still works
    d, parent, K, kw2, want = CC.case("single")
    same(hd.cluster_parts(d, parent, K, **kw2), want)
