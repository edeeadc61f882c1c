"""PBD_CONV_MFMA_F64: the filter bank of a T = double handle on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).
Responses differ from the reference's summation order by fp64 rounding only, so they are held to 1e-10 absolute on
unit-scale inputs, and the detections (scores compared as float32) equal the oracle's double path."""
import numpy as np
import pytest

from partsbaseddetector_amd import synth
from partsbaseddetector_amd import model as M

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def det_mod():
    from partsbaseddetector_amd import detector
    return detector


def _f64_handle(det_mod, flat, **kw):
    from partsbaseddetector_amd import _lib
    return det_mod.Handle(flat, device=0, real_type=_lib.REAL_F64, conv_mode=_lib.CONV_MFMA_F64, **kw)


def _f64_detector(det_mod, **kw):
    from partsbaseddetector_amd import _lib
    return det_mod.PartsBasedDetector(device=0, dtype=np.float64, conv_mode=_lib.CONV_MFMA_F64, **kw)


def _compare_candidates(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (g.level, g.component, g.root[1], g.root[0]) == (w["level"], w["component"], w["root_y"], w["root_x"])
        assert np.array_equal(g.parts, w["parts"]), (g.parts, w["parts"])
        assert np.float32(g.score()) == np.float32(w["score"])


def _records(cands):
    return [(c.frame, c.level, c.component, c.root, c.score(), c.parts.tobytes()) for c in cands]


def _single(cands):
    return [(c.level, c.component, c.root, c.score(), c.parts.tobytes()) for c in cands]


def test_matrix_modes_of_other_real_types_are_refused(det_mod):
    from partsbaseddetector_amd import _lib
    from partsbaseddetector_amd._lib import PbdError
    flat = M.synthetic_tiny_model().flatten()
    for mode in (_lib.CONV_MFMA, _lib.CONV_MFMA_F16):              # unchanged: the float matrix modes refuse T = double
        with pytest.raises(PbdError) as e:
            det_mod.Handle(flat, device=0, real_type=_lib.REAL_F64, conv_mode=mode)
        assert e.value.code == -2 and "PBD_REAL_F32" in str(e.value)
    with pytest.raises(PbdError) as e:
        det_mod.Handle(flat, device=0, real_type=_lib.REAL_F32, conv_mode=_lib.CONV_MFMA_F64)
    assert e.value.code == -2 and "PBD_REAL_F64" in str(e.value)


def test_conv_pdf_ragged_levels(det_mod, oracle):
    """test_conv_pdf's level list: an empty level, 1 x 1, maps smaller than the filter, widths of 64 and more, a non-zero
    channel 31 inside the image."""
    flat = M.synthetic_tiny_model().flatten()
    hd = _f64_handle(det_mod, flat)
    conv = det_mod.SpatialConvolutionEngine(hd)
    rng = np.random.default_rng(5)
    dims = [(37, 45), (8, 33), (3, 2), (1, 1), (0, 5), (12, 70), (5, 64), (4, 65), (9, 130), (7, 201), (66, 97)]
    feats = [rng.random((h, w * 32)) * 0.4 for h, w in dims]
    for f in feats:
        if f.size:
            f.reshape(f.shape[0], -1, 32)[:, :, 31] = 0.0
    feats[1].reshape(8, 33, 32)[:, :, 31] = 0.3
    feats[8].reshape(9, 130, 32)[:, :, 31] = 0.2
    got = conv.pdf(feats)
    worst = 0.0
    for (h, w), f, g in zip(dims, feats, got):
        assert g.dtype == np.float64 and g.shape == (flat.nfilters, h, w)
        if h * w == 0:
            continue
        err = float(np.abs(g - oracle.responses(flat, f)).max())
        assert err <= TOL, (h, w, err)
        worst = max(worst, err)
    print(f"PBD_CONV_MFMA_F64 pdf: max |response - reference| = {worst:.3g}")
    hd.close()


def test_filter_counts_across_tiles_and_passes(det_mod, oracle):
    """170 filters: 11 M-tiles of 16 (the last one ragged) in three passes."""
    flat = M.synthetic_tiny_model().flatten()
    hd = _f64_handle(det_mod, flat)
    conv = det_mod.SpatialConvolutionEngine(hd)
    rng = np.random.default_rng(6)
    filters = [rng.standard_normal((5, 5 * 32)) * 0.1 for _ in range(170)]
    conv.setFilters(filters)
    feats = [rng.random((20, 41 * 32)), rng.random((3, 70 * 32))]
    for feat, got in zip(feats, conv.pdf(feats)):
        assert got.shape == (170, feat.shape[0], feat.shape[1] // 32)
        for f in (0, 15, 16, 159, 160, 169):
            assert np.abs(got[f] - oracle.conv(feat, filters[f])).max() <= TOL, f
    hd.close()


@pytest.mark.parametrize("ksizes,nmix,pa", [([5, 3, 7, 4], 3, [0, 1, 1, 2]), ([9, 8], 2, [0, 1, 1, 2]), ([12, 5], 3, [0, 1, 1, 2]),
                                            ([31], 1, [0, 1])])
def test_filter_sizes(det_mod, oracle, ksizes, nmix, pa):
    """Several sizes in one bank (one launch per size class), large filters (smaller channel blocks) and 31 x 31, the
    largest size: responses at the first and last level, and the candidates of the oracle's double path."""
    model = M.synthetic_model(seed=31 + nmix, pa=pa, nmix=nmix, ksize=ksizes, interval=5, thresh=-1e9, name="sizes")
    flat = model.flatten()
    assert sorted(set(int(k) for k in flat.filter_ksize)) == sorted(set(ksizes))
    im = synth.synthetic_frame(43, 140, 120, 3)
    want = oracle.detect(flat, im, dtype=np.float64)
    model.thresh = float(np.sort([w["score"] for w in want])[-min(50, len(want))])
    flat = model.flatten()
    want = oracle.detect(flat, im, dtype=np.float64)
    det = _f64_detector(det_mod)
    det.distributeModel(model)
    got = det.detect(im)
    _compare_candidates(got, want)
    feats, _ = oracle.features_pyramid(flat, im, dtype=np.float64)
    for l in (0, len(feats) - 1):
        H, W = feats[l].shape[0], feats[l].shape[1] // 32
        r = det.hd.get_stage(1, 0, l, H, W)
        wr = oracle.responses(flat, feats[l])
        assert r.dtype == np.float64 and np.abs(r - wr).max() <= TOL, (l, np.abs(r - wr).max())
    det.hd.close()


@pytest.mark.parametrize("shape,thresh", [((160, 120), 17.9), ((480, 640), 18.9)])
def test_person_model_end_to_end(det_mod, oracle, shape, thresh):
    model = M.synthetic_person_model(thresh=thresh)
    det = _f64_detector(det_mod)
    det.distributeModel(model)
    im = synth.synthetic_frame(21, shape[0], shape[1], 3)
    got = det.detect(im)
    want = oracle.detect(model.flatten(), im, dtype=np.float64)
    assert len(want) > 0
    _compare_candidates(got, want)
    det.hd.close()


def test_every_entry_point(det_mod):
    """Batches, submit / wait, device-resident frames, device NMS, DP chunks and level sharding in this mode give the records
    of single detect() calls on a handle in the same mode."""
    import ctypes as C
    from partsbaseddetector_amd import _lib
    model = M.synthetic_person_model(thresh=17.9)
    frames = [synth.synthetic_frame(60 + i, 120, 160, 3) for i in range(8)]
    det = _f64_detector(det_mod, max_batch=8)
    det.distributeModel(model)
    single = [_single(det.detect(f)) for f in frames]
    assert sum(len(s) for s in single) > 8
    want = [(i,) + r for i, s in enumerate(single) for r in s]
    assert _records(det.detect_batch(frames)) == want
    det.submit_batch(frames)
    assert _records(det.wait_batch()) == want
    hip = det.hd.lib           # device memory from the runtime the library is bound to, not a second one in this process
    for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                       ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
        getattr(hip, name).argtypes = args
    packed = np.ascontiguousarray(np.stack(frames))
    d_frames = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_frames), packed.nbytes) == 0
    try:
        assert hip.hipMemcpy(d_frames, packed.ctypes.data, packed.nbytes, 1) == 0          # hipMemcpyHostToDevice
        assert _records(det.detect_batch_device(d_frames.value, 8, 120, 160, 3)) == want
    finally:
        hip.hipFree(d_frames)
    det.hd.set_debug_option(_lib.DP_BUDGET_MB, 1)                  # the dynamic program in chunks of one frame
    assert _records(det.detect_batch(frames)) == want
    det.hd.set_debug_option(_lib.DP_BUDGET_MB, 0)
    det.hd.close()

    nms = _f64_detector(det_mod, max_batch=8, nms=0.1)
    nms.distributeModel(model)
    mirror = _f64_detector(det_mod)
    mirror.distributeModel(model)
    per_frame = []
    for i, f in enumerate(frames):
        ref = mirror.detect(f)
        det_mod.Candidate.sort(ref)
        det_mod.Candidate.nonMaximaSuppression(f.shape, ref, float(np.float32(0.1)))
        got = nms.detect(f)
        assert _single(got) == _single(ref), i
        per_frame += [(i,) + r for r in _single(got)]
    assert _records(nms.detect_batch(frames)) == per_frame
    mirror.hd.close()
    nms.hd.close()

    im = synth.synthetic_frame(3, 240, 320, 3)
    det = _f64_detector(det_mod)
    det.distributeModel(model)
    full = sorted(_single(det.detect(im)))
    assert len(full) > 0
    got = []
    for rank in range(2):
        det.hd.set_level_shard(rank, 2)
        got += _single(det.detect(im))
    assert sorted(got) == full
    det.hd.close()


def test_handles_on_two_devices_in_one_process(det_mod, oracle):
    """The dynamic-LDS limit is a per-device property of a kernel: a handle on device 0, then one on device 1, in one process,
    both within TOL of the oracle.  19 x 19 filters (4-channel blocks, 61 KB per tile) and 7 x 7 filters (16-channel blocks,
    75 KB: above the 64 KB a kernel may ask for by default)."""
    import ctypes as C
    from partsbaseddetector_amd import _lib
    ndev = C.c_int(0)
    assert _lib.load().hipGetDeviceCount(C.byref(ndev)) == 0
    if ndev.value < 2:
        pytest.skip("one device visible")
    flat = M.synthetic_tiny_model().flatten()
    rng = np.random.default_rng(19)
    feat = rng.random((40, 41 * 32)) * 0.4
    filters = [rng.standard_normal((k, k * 32)) * 0.1 for k in (19, 19, 7)]
    want = [oracle.conv(feat, w) for w in filters]
    for device in (0, 1):
        hd = det_mod.Handle(flat, device=device, real_type=_lib.REAL_F64, conv_mode=_lib.CONV_MFMA_F64)
        conv = det_mod.SpatialConvolutionEngine(hd)
        conv.setFilters(filters)
        got = conv.pdf([feat])[0]
        assert got.shape == (3, 40, 41)
        for f in range(3):
            err = float(np.abs(got[f] - want[f]).max())
            print(f"device {device} filter {f}: max |response - reference| = {err:.3g}")
            assert err <= TOL, (device, f, err)
        hd.close()


def test_set_filters_on_a_handle_in_this_mode(det_mod, oracle):
    """Replacing the bank with another size mix works; a refused bank (33 x 33) keeps the old responses bit for bit."""
    from partsbaseddetector_amd._lib import PbdError
    flat = M.synthetic_tiny_model().flatten()
    hd = _f64_handle(det_mod, flat)
    conv = det_mod.SpatialConvolutionEngine(hd)
    rng = np.random.default_rng(9)
    feat = rng.random((17, 29 * 32)) * 0.4
    filters = [rng.standard_normal((k, k * 32)) * 0.1 for k in (3, 6, 3, 11, 1, 6, 6)]
    conv.setFilters(filters)
    before = conv.pdf([feat])[0]
    for f, w in enumerate(filters):
        assert np.abs(before[f] - oracle.conv(feat, w)).max() <= TOL, f
    with pytest.raises(PbdError) as e:
        conv.setFilters([rng.standard_normal((33, 33 * 32)) for _ in range(4)])
    assert e.value.code == -2
    conv._nfilters = len(filters)
    after = conv.pdf([feat])[0]
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    hd.close()
