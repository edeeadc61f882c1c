"""The in-place model update (pbd_set_model_vector, pbd_set_model_vector_device, pbd_qp_apply, pbd_set_thresh): after a
successful call the handle cannot be told apart from a handle created from Model.from_vector(w) with the same config.

"Equal" below means: the records of pbd_detect_frames on two synthetic frames are equal byte for byte (and both frames give
records), and the pbd_get_stage response and score planes of one interior level and of the smallest level are equal byte for
byte.  The reference of every comparison is a fresh handle, never a stored value."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import qp as Q
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
LOW = -1e9          # a threshold every root passes: both frames give records


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def shared_model():
    m = M.synthetic_tiny_model(thresh=LOW)
    m.filterid[0][2] = list(m.filterid[0][1])
    m.validate()
    return m


def mixed_model(ksizes, nmix):
    return M.synthetic_model(seed=29 + nmix, pa=[0, 1, 1, 2], nmix=nmix, ksize=ksizes, interval=5, thresh=LOW, name="large")


def handle(model, dtype=np.float32, mode=_lib.CONV_EXACT, max_batch=2):
    return detector.Handle(model, device=0, real_type=REAL[dtype], conv_mode=mode, max_candidates=1 << 18, max_batch=max_batch)


def records(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], _lib.DEPTH_CODE[fr[0].dtype], buf.ctypes.data,
                                      hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def two_frames(shape):
    return [synth.synthetic_frame(61 + k, shape[0], shape[1]) for k in range(2)]


def observe(hd, frames):
    """(records, planes) of a detect of `frames`: what "equal" compares"""
    rec = records(hd, frames)
    assert set(np.unique(rec[:, 0])) == {0, 1}, "both frames give records"
    plan = hd.plan(*frames[0].shape[:2])
    planes = []
    for l in (plan["nlevels"] // 2, plan["nlevels"] - 1):
        r, c = int(plan["feat_rows"][l]), int(plan["feat_cols"][l])
        assert r > 0 and c > 0
        planes += [hd.get_stage(_lib.STAGE_RESPONSES, 0, l, r, c), hd.get_stage(_lib.STAGE_ROOTV, 0, l, r, c)]
    return rec, planes


def assert_equal(a, b):
    (ra, pa), (rb, pb) = a, b
    assert ra.shape == rb.shape and ra.tobytes() == rb.tobytes()
    for u, v in zip(pa, pb):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()


def new_vector(hd, flat, seed=7, linear=True):
    """the handle's vector plus seeded noise on every block; quadratic deformation terms stay positive; channel 31 of every
    filter is set to a mix of nonzero, +0.0 and -0.0 so that the border table's zero skip and order matter"""
    rng = np.random.default_rng(seed)
    w = hd.model_vector().astype(np.float64)
    nb, nd = len(flat.biasw), len(flat.defw)
    fbase = nb + 4 * nd
    w[:nb] += rng.normal(0, 0.05, nb)
    d = w[nb:fbase].reshape(nd, 4)
    d[:, [0, 2]] += np.abs(rng.normal(0, 0.002, (nd, 2)))
    if linear:
        d[:, [1, 3]] += rng.normal(0, 0.004, (nd, 2))
    w[fbase:] += rng.normal(0, 0.01, len(w) - fbase)
    pattern = np.array([0.03, 0.0, -0.0, -0.02, 0.0, 0.015, -0.0, 0.0, -0.04, 0.025])
    for f in range(flat.nfilters):
        k = int(flat.filter_ksize[f])
        o = fbase + int(flat.filter_offset[f])
        w[o + 31: o + k * k * 32: 32] = np.resize(np.roll(pattern, f), k * k)
    return w.astype(hd.dtype)


def rounded(w, flat, dtype):
    """w as pbd_create rounds Model.from_vector(w): bias and deformation values through float32, filters to T"""
    out = np.asarray(w).astype(dtype)
    n = len(flat.biasw) + 4 * len(flat.defw)
    out[:n] = np.asarray(w[:n]).astype(np.float32).astype(dtype)
    return out


CASES = {
    "person-exact": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float32, _lib.CONV_EXACT),
    "person-fma": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float32, _lib.CONV_FMA),
    "person-mfma": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float32, _lib.CONV_MFMA),
    "person-mfma-f16": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float32, _lib.CONV_MFMA_F16),
    "person-f64-exact": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float64, _lib.CONV_EXACT),
    "person-f64-mfma": (lambda: M.synthetic_person_model(thresh=LOW), (120, 160), np.float64, _lib.CONV_MFMA_F64),
    "tiny-f32": (lambda: M.synthetic_tiny_model(thresh=LOW), (72, 96), np.float32, _lib.CONV_EXACT),
    "tiny-f64": (lambda: M.synthetic_tiny_model(thresh=LOW), (72, 96), np.float64, _lib.CONV_EXACT),
    "mixed-f32-9-12-5": (lambda: mixed_model([9, 12, 5], 3), (140, 120), np.float32, _lib.CONV_EXACT),
    "mixed-f64-9-8": (lambda: mixed_model([9, 8], 2), (140, 120), np.float64, _lib.CONV_EXACT),
    "mixed-f64-9-8-mfma": (lambda: mixed_model([9, 8], 2), (140, 120), np.float64, _lib.CONV_MFMA_F64),
    "shared-seq": (shared_model, (72, 96), np.float32, _lib.CONV_EXACT),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_update_equals_fresh_handle(name):
    make, shape, dtype, mode = CASES[name]
    model = make()
    flat = model.flatten()
    frames = two_frames(shape)
    hd = handle(model, dtype, mode)
    before = observe(hd, frames)
    w = new_vector(hd, flat)
    hd.set_model_vector(w)
    assert hd.model_vector().tobytes() == rounded(w, flat, dtype).tobytes()
    got = observe(hd, frames)
    fresh = handle(model.from_vector(w), dtype, mode)
    assert fresh.model_vector().tobytes() == hd.model_vector().tobytes()
    want = observe(fresh, frames)
    assert_equal(got, want)
    assert got[0].tobytes() != before[0].tobytes()          # and the update changed what is detected
    hd.close(); fresh.close()


def test_variant_flags_both_ways():
    """linear deformation terms +0.0 (the distance transform's variant without them) -> nonzero -> back"""
    model = M.synthetic_person_model(thresh=LOW)
    flat = model.flatten()
    assert not np.any(flat.defw[:, [1, 3]]) and not np.any(np.signbit(flat.defw[:, [1, 3]]))
    frames = two_frames((120, 160))
    hd = handle(model)
    w0 = hd.model_vector()
    original = observe(hd, frames)
    w1 = new_vector(hd, flat, seed=11, linear=True)
    nb = len(flat.biasw)
    assert np.all(w1[nb:nb + 4 * len(flat.defw)].reshape(-1, 4)[:, [1, 3]] != 0)
    hd.set_model_vector(w1)
    assert hd.model_vector().tobytes() == w1.tobytes()
    fresh = handle(model.from_vector(w1))
    assert_equal(observe(hd, frames), observe(fresh, frames))
    fresh.close()
    hd.set_model_vector(w0)
    assert hd.model_vector().tobytes() == w0.tobytes()
    assert_equal(observe(hd, frames), original)
    hd.close()


LAT = dict(shape=(72, 96), box=[20, 16, 60, 56], overlap=0.3)


def latent(hd, flat, frames):
    boxes = [[LAT["box"]] * flat.max_parts for _ in frames]
    rec, found = hd.detect_latent(frames, boxes, LAT["overlap"])
    assert found.all()
    hdr, vals = hd.examples(rec)
    for i in range(len(rec)):
        vals[i, hdr[i, 3]:] = 0                      # values past nvalues are not written (include/pbd.h)
    return rec, hdr, vals


def shared_reversed_model():
    """filter ids shared between parts AND out of order: part 1 uses part 2's filters reversed, so the latent twin's filter gm
    is not block gm of the vector"""
    m = M.synthetic_tiny_model(thresh=-1.0)
    m.filterid[0][1] = list(m.filterid[0][2])[::-1]
    m.validate()
    return m


@pytest.mark.parametrize("which", ["tiny", "shared", "shared-reversed"])
@pytest.mark.parametrize("twin_first", [True, False])
def test_latent_twin_follows(twin_first, which):
    model = {"tiny": lambda: M.synthetic_tiny_model(thresh=-1.0), "shared": shared_model, "shared-reversed": shared_reversed_model}[which]()
    flat = model.flatten()
    frames = [synth.synthetic_frame(40 + k, *LAT["shape"]) for k in range(4)]
    hd = handle(model, max_batch=4)
    if twin_first:
        old = latent(hd, flat, frames)               # the twin exists before the update
    w = new_vector(hd, flat, seed=5)
    hd.set_model_vector(w)
    got = latent(hd, flat, frames)
    fresh = handle(model.from_vector(w), max_batch=4)
    want = latent(fresh, flat, frames)
    for u, v in zip(got, want):
        assert u.shape == v.shape and u.tobytes() == v.tobytes()
    if twin_first:
        assert got[0].tobytes() != old[0].tobytes()
    assert_equal(observe(hd, frames[:2]), observe(fresh, frames[:2]))
    hd.close(); fresh.close()


def test_device_forms_equal_host_form():
    import torch
    model = M.synthetic_tiny_model(thresh=LOW)
    flat = model.flatten()
    frames = two_frames((72, 96))
    base = handle(model)
    rng = np.random.default_rng(3)
    w64 = new_vector(base, flat, seed=9).astype(np.float64)
    w64[len(flat.biasw) + 4 * len(flat.defw):] += rng.normal(0, 1e-9, len(w64) - len(flat.biasw) - 4 * len(flat.defw))
    assert not np.array_equal(w64, w64.astype(np.float32).astype(np.float64))     # the F64 source does not fit float32
    w32 = w64.astype(np.float32)
    host = handle(model)
    host.set_model_vector(w32)
    want = observe(host, frames)
    for src in (w64, w32):
        hd = handle(model)
        t = torch.from_numpy(src).cuda()
        torch.cuda.synchronize()
        hd.set_model_vector_device(t.data_ptr(), src.dtype)
        assert hd.model_vector().tobytes() == w32.tobytes()
        assert_equal(observe(hd, frames), want)
        hd.close()
    base.close(); host.close()


def test_qp_apply_round_and_second_round():
    """the mining steps of a training round for the tiny model, QP.apply instead of a new detector, then a second round on
    the same handle"""
    import torch
    rows, cols = LAT["shape"]
    model = M.synthetic_tiny_model(thresh=-1.0)
    flat = model.flatten()
    det = detector.PartsBasedDetector(max_batch=4)
    det.distributeModel(model)
    hd = det.hd
    frames = [synth.synthetic_frame(40 + k, rows, cols) for k in range(4)]
    negs = [synth.synthetic_frame(90 + k, rows, cols, kind="noise") for k in range(2)]
    boxes = [[LAT["box"]] * flat.max_parts for _ in frames]
    q = det.qp(512)
    hw, vw = hd.example_stride()
    st = hd.stride

    def push(rec, label, id_base):
        pay = torch.zeros(1 + len(rec) * st, dtype=torch.int32, device="cuda")
        pay[0] = len(rec)
        pay[1:] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
        dh = torch.zeros(len(rec) * hw, dtype=torch.int32, device="cuda")
        dv = torch.zeros(len(rec) * vw, dtype=torch.float32, device="cuda")
        hd.examples_device(pay.data_ptr(), len(rec), 0, dh.data_ptr(), dv.data_ptr())
        q.add_device(hd, pay.data_ptr(), len(rec), dh.data_ptr(), dv.data_ptr(), label, id_base)

    def mine(id_base):
        cands, found = det.detectLatent(frames, boxes, LAT["overlap"])
        assert found.all()
        push(hd.pack_candidates(cands), 1, id_base)
        if id_base == 0:
            q.fix()
        neg_rec = records(hd, negs)
        assert len(neg_rec) > 10
        push(neg_rec[:150], -1, id_base + 100)

    mine(0)
    q.prune()
    s = q.opt(tol=0.05, iter=500, seed=1)
    assert s["converged"]
    det.updateModel(q)
    w = q.weights()
    assert det.modelVector().tobytes() == w.astype(np.float32).tobytes()
    with pytest.raises(PbdError) as e:                       # the resident result was the old weights'
        hd.examples(np.zeros((1, st), np.int32))
    assert e.value.code == -5
    fresh = handle(model.from_vector(w), max_batch=4)
    two = frames[:2]
    assert_equal(observe(hd, two), observe(fresh, two))
    assert det.model().to_vector(np.float32).tobytes() == w.astype(np.float32).tobytes()
    fresh.close()
    # a second round on the same handle
    mine(1000)
    s = q.opt(tol=0.05, iter=1000, seed=2)
    assert s["converged"] and 1 - s["lb"] / s["ub"] < 0.05
    q.apply(hd)
    w2 = q.weights()
    assert hd.model_vector().tobytes() == w2.astype(np.float32).tobytes()
    fresh = handle(model.from_vector(w2), max_batch=4)
    assert_equal(observe(hd, two), observe(fresh, two))
    fresh.close()


def test_set_thresh():
    model = M.synthetic_tiny_model(thresh=LOW)
    frames = two_frames((72, 96))
    hd = handle(model)
    rec = records(hd, frames)
    thresh = float(np.median(rec[:, 5].copy().view(np.float32)))
    hd.set_thresh(thresh)
    got = records(hd, frames)
    assert 0 < len(got) < len(rec) and set(np.unique(got[:, 0])) == {0, 1}
    other = M.synthetic_tiny_model(thresh=thresh)
    fresh = handle(other)
    assert got.tobytes() == records(fresh, frames).tobytes()
    assert hd.current_model().thresh == np.float32(thresh)
    hd.close(); fresh.close()


def test_refusals_leave_the_handle_unchanged():
    import torch
    model = M.synthetic_tiny_model(thresh=LOW)
    flat = model.flatten()
    frames = two_frames((72, 96))
    hd = handle(model, max_batch=2)
    w0 = hd.model_vector()
    before = observe(hd, frames)

    def unchanged():
        assert hd.model_vector().tobytes() == w0.tobytes()
        assert_equal(observe(hd, frames), before)

    def refused(code, call, *args):
        with pytest.raises(PbdError) as e:
            call(*args)
        assert e.value.code == code, e.value

    # a deformation whose element 0 is zero: host and device forms
    bad = new_vector(hd, flat, seed=2)
    bad[len(flat.biasw) + 4 * 1] = 0.0
    refused(-1, hd.set_model_vector, bad)
    unchanged()
    t = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    refused(-1, hd.set_model_vector_device, t.data_ptr(), np.float32)
    unchanged()
    refused(-1, hd.set_model_vector_device, t.data_ptr(), np.int32)
    assert hd.lib.pbd_set_model_vector_device(hd.h, t.data_ptr(), 7) == -1
    assert hd.lib.pbd_set_model_vector(hd.h, None) == -1
    assert hd.lib.pbd_set_model_vector_device(hd.h, None, _lib.REAL_F32) == -1
    # a QP of another layout
    person = handle(M.synthetic_person_model(thresh=LOW))
    q = Q.QP(person, 4)
    refused(-1, q.apply, hd)
    assert hd.lib.pbd_qp_apply(q.q, None) == -1
    unchanged()
    person.close()
    # while a batch is in flight
    good = new_vector(hd, flat, seed=4)
    ims = [np.ascontiguousarray(f) for f in frames]
    arr = _lib.ptr_array(ims)
    rows, cols, cn = ims[0].shape
    hd.check(hd.lib.pbd_detect_batch_submit(hd.h, 2, arr, rows, cols, cn, ims[0].strides[0]))
    refused(-5, hd.set_model_vector, good)
    refused(-5, hd.set_thresh, 0.0)
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch_wait(hd.h, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    assert n.value > 0
    unchanged()
    # pbd_examples right after an update
    hd.set_model_vector(good)
    refused(-5, hd.examples, before[0][:1])
    hd.set_model_vector(w0)
    unchanged()
    # after pbd_conv_set_filters with a smaller bank the model vector no longer describes the bank
    eng = detector.SpatialConvolutionEngine(hd)
    eng.setFilters([np.asarray(f, np.float32) for f in model.filtersw[:2]])
    refused(-5, hd.set_model_vector, good)
    assert hd.model_vector().tobytes() == w0.tobytes()
    eng.setFilters([np.asarray(f, np.float32) for f in model.filtersw])
    unchanged()
    hd.close()
