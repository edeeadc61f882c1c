"""The scale NMS on the GPU: the detect path (pbd_set_scale_nms) and the list form (pbd_scale_nms*), each against the numpy
yardstick of scalenms.py, record for record and word for word.

Detect path: the yardstick is a list of the same handle with the step off (the `base`), filtered by scalenms.keep_records -- all
pairs over the records' root rectangles -- with the scores taken from PBD_STAGE_ROOTV in the handle's T.  With root NMS or depth
pruning on, the base is the list those filters leave; with top-K on, the result must be top-K of the survivors.  The inputs'
conditions (the pinned counts, the constant frame's cross-level ties) are checked on the CPU oracle in test_scale_nms_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, detector, synth, topk
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import scalenms as S
from partsbaseddetector_amd.detector import PbdError

import scale_nms_cases as T

pytestmark = pytest.mark.gpu
THRESH = -1.0
MIXED_SHAPES = ((48, 64), (60, 50), (40, 72))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def records(hd, frames):
    """the raw records of one call: pbd_detect_batch for equal sizes, pbd_detect_frames for mixed ones"""
    fr = [np.ascontiguousarray(f) for f in frames]
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    if len({f.shape for f in fr}) == 1:
        rows, cols, cn = fr[0].shape
        hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                         hd.max_candidates, C.byref(n)))
    else:
        descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
        hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, fr[0].shape[2], 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def rootv_scores(hd, frames, rec):
    """rootv at every record's root cell from the resident result of a call on `frames`, in the handle's T"""
    planes = {}
    out = []
    for r in rec:
        f, l = int(r[0]), int(r[2])
        if (f, l) not in planes:
            pl = hd.plan(frames[f].shape[0], frames[f].shape[1])
            planes[(f, l)] = hd.get_stage(_lib.STAGE_ROOTV, f, l, int(pl["feat_rows"][l]), int(pl["feat_cols"][l]))
        out.append(planes[(f, l)][int(r[1])][int(r[4]), int(r[3])])
    return np.array(out)


def with_scale_nms(hd, dl, frames):
    hd.set_scale_nms(dl)
    try:
        return records(hd, frames)
    finally:
        hd.set_scale_nms(None)


def filtered(base, dl, scores=None):
    return base[S.keep_records(base, dl, scores)]


def make(model, dtype=np.float32, **kw):
    det = detector.PartsBasedDetector(device=0, dtype=dtype, **kw)
    det.distributeModel(model)
    return det


@pytest.fixture(scope="module")
def tiny():
    model = M.synthetic_tiny_model(thresh=THRESH)
    det = make(model, max_batch=4)
    frames = {shape: synth.synthetic_frame(5, shape[0], shape[1], 3) for shape in T.SHAPES}
    yield model, det, det.hd, frames
    det.hd.close()


# ---- the detect path against the yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=["f32", "f64"])
def test_detect_equals_the_filtered_off_run(dtype):
    model = M.synthetic_tiny_model(thresh=THRESH)
    det = make(model, dtype)
    hd = det.hd
    try:
        for shape, counts in zip(T.SHAPES, ((446, [22, 7, 4, 2]), (2422, [87, 27, 19, 15]))):
            fr = [synth.synthetic_frame(5, shape[0], shape[1], 3)]
            base = records(hd, fr)
            sc = rootv_scores(hd, fr, base)
            assert sc.dtype == dtype and np.array_equal(sc.astype(np.float32), base[:, 5].copy().view(np.float32))
            got = []
            for dl in T.DLS:
                on = with_scale_nms(hd, dl, fr)
                assert np.array_equal(on, filtered(base, dl, sc)), (shape, dl)
                got.append(len(on))
            if dtype == np.float32:                 # the CPU oracle's counts (test_scale_nms_cpu.py)
                assert (len(base), got) == counts
        # the constant frame with every cell eligible: ties across cells and levels decide
        hd.set_thresh(-1e30)
        fr = [T.constant_frame()]
        base = records(hd, fr)
        sc = rootv_scores(hd, fr, base)
        assert len(base) == 446
        for dl in (0, 1, 2, 5):
            assert T.tied_neighbour_pairs(base, dl)[1] > 0 or dl == 0
            on = with_scale_nms(hd, dl, fr)
            assert np.array_equal(on, filtered(base, dl, sc)), dl
            assert 0 < len(on) < 20
        # off again: the bytes of a handle that never had the step on
        fresh = detector.Handle(model, device=0, real_type=_lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64)
        try:
            fresh.set_thresh(-1e30)
            assert np.array_equal(records(hd, fr), records(fresh, fr))
        finally:
            fresh.close()
    finally:
        hd.close()


def test_composition_with_root_nms_top_k_and_set_nms(tiny):
    model, det, hd, frames = tiny
    fr = [frames[(96, 128)]]
    try:
        hd.set_root_nms(2)
        base = records(hd, fr)
        assert len(base) == 87
        for dl, n in zip(T.DLS, (87, 40, 30, 24)):
            on = with_scale_nms(hd, dl, fr)
            assert np.array_equal(on, filtered(base, dl)) and len(on) == n, dl
        # K is taken among the scale-space maxima
        surv = filtered(base, 1)
        for k in (1, 5, 39, 40, 100):
            hd.set_top_k(k)
            got = with_scale_nms(hd, 1, fr)
            assert np.array_equal(got, topk.top_k_records_ref(surv, k)), k
            assert len(got) == min(k, 40)
        hd.set_top_k(0)
        hd.set_root_nms(0)
        base = records(hd, fr)
        surv = filtered(base, 2)
        hd.set_top_k(7)
        assert np.array_equal(with_scale_nms(hd, 2, fr), topk.top_k_records_ref(surv, 7))
        hd.set_top_k(0)
        # pbd_set_nms sees only the kept list
        want = hd.suppress([(96, 128)], 0.1, surv)
        hd.set_nms(0.1)
        got = with_scale_nms(hd, 2, fr)
        assert 1 <= len(want) <= len(surv) and np.array_equal(got, want)
    finally:
        hd.set_nms(None)
        hd.set_top_k(0)
        hd.set_root_nms(0)


def test_composition_with_depth_pruning(tiny):
    model, det, hd, frames = tiny
    fr = [frames[(96, 128)]]
    raw = records(hd, fr)
    widths = sorted({int(w) for w in raw[:, 10]})
    rng = np.random.default_rng(3)
    vals = np.rint(np.array([500.0 * 40.0 / w for w in widths[::2]]))
    depth = vals[np.kron(rng.integers(0, len(vals), (24, 32)), np.ones((4, 4), np.int64))].astype(np.uint16)
    hd.set_depth_prune(500.0, 40.0, 0.02)
    try:
        hd.bind_depth([depth])
        base = records(hd, fr)
        assert 10 <= len(base) < len(raw)
        for dl in (1, 5):
            hd.bind_depth([depth])
            on = with_scale_nms(hd, dl, fr)
            assert np.array_equal(on, filtered(base, dl)) and len(on) < len(base), dl
        hd.set_root_nms(2)
        hd.bind_depth([depth])
        base = records(hd, fr)
        hd.bind_depth([depth])
        assert np.array_equal(with_scale_nms(hd, 2, fr), filtered(base, 2))
    finally:
        hd.set_root_nms(0)
        hd.set_depth_prune(None)


def test_padding_and_the_fine_octave():
    model = M.synthetic_tiny_model(thresh=THRESH)
    im = synth.synthetic_frame(5, 48, 64, 3)
    for setup in ("padding", "fine", "both"):
        det = make(model)
        hd = det.hd
        try:
            if setup in ("padding", "both"):
                hd.set_padding(2, 2)
            if setup in ("fine", "both"):
                hd.set_fine_octave(True)
            base = records(hd, [im])
            if setup != "fine":
                assert (base[:, 8] < 0).any() and (base[:, 3] < 2).any()    # roots on the pad
            if setup != "padding":
                assert base[:, 2].max() >= hd.flat.model.interval * 2       # the longer level list
            assert len(base) > 446
            for dl in (0, 1, 5):
                on = with_scale_nms(hd, dl, [im])
                assert np.array_equal(on, filtered(base, dl)) and 0 < len(on) < len(base), (setup, dl)
        finally:
            hd.close()


def test_three_components_and_roots_of_different_filter_sides():
    model = M.synthetic_model(seed=17, pa=[0, 1, 1], nmix=2, ncomponents=3, ksize=[5, 3, 7, 4], interval=5, thresh=-0.5,
                              linear_def=True, name="three")
    assert len({k for ks in T.root_ksizes(model) for k in ks}) >= 3
    det = make(model)
    hd = det.hd
    try:
        im = synth.synthetic_frame(5, 64, 80, 3)
        base = records(hd, [im])
        assert len(np.unique(base[:, 1])) == 3 and len({(int(r[2]), int(r[10])) for r in base if r[2] == 0}) >= 3
        for dl in (0, 1, 5):
            on = with_scale_nms(hd, dl, [im])
            want = filtered(base, dl)
            assert np.array_equal(on, want) and 0 < len(on) < len(base), dl
        # other components take part: within one component alone more would survive
        alone = sum(int(S.keep_records(base[base[:, 1] == c], 0).sum()) for c in range(3))
        assert alone > len(filtered(base, 0))
    finally:
        hd.close()


def test_equal_batch_submit_wait_mixed_sizes_and_pool(tiny):
    model, det, hd, frames = tiny
    batch = [synth.synthetic_frame(5 + i, 48, 64, 3) for i in range(3)] + [T.constant_frame()]
    base = records(hd, batch)
    want = filtered(base, 1)
    assert len(np.unique(want[:, 0])) == 4 and len(want) < len(base)
    assert np.array_equal(with_scale_nms(hd, 1, batch), want)
    for f in range(4):                                  # frames do not meet: each is its own single-frame result
        one = with_scale_nms(hd, 1, [batch[f]])
        assert np.array_equal(one[:, 1:], want[want[:, 0] == f][:, 1:])
    # _submit / _wait: latched at submit, refused in flight
    det.setScaleNMS(1)
    try:
        det.submit_batch(batch)
        assert hd.lib.pbd_set_scale_nms(hd.h, 0, 0) == -5
        assert hd.lib.pbd_scale_nms(hd.h, 1, 1, None, 0, 0, None, 0, C.byref(C.c_int())) == -5
        buf, n = det.wait_batch(raw=True)
        assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), want)
    finally:
        det.setScaleNMS(None)
    # mixed sizes: a frame's neighbours are its own levels
    mixed = [synth.synthetic_frame(41 + i, r, c, 3) for i, (r, c) in enumerate(MIXED_SHAPES)]
    base_m = records(hd, mixed)
    for dl in (0, 2, 255):
        on = with_scale_nms(hd, dl, mixed)
        assert np.array_equal(on, filtered(base_m, dl)) and len(on) < len(base_m), dl
    one = with_scale_nms(hd, 2, [mixed[1]])
    on = with_scale_nms(hd, 2, mixed)
    assert np.array_equal(one[:, 1:], on[on[:, 0] == 1][:, 1:])
    pool = detector.DetectorPool(model, n=2, device=0, max_batch=4)
    try:
        pool.setScaleNMS(1)
        for _ in range(2):
            pool.submit_batch(batch)
        for _ in range(2):
            buf, n = pool.wait_batch(raw=True)
            assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), want)
    finally:
        pool.close()


def test_detect_regions(tiny):
    import torch
    model, det, hd, frames = tiny
    image = torch.from_numpy(synth.synthetic_frame(9, 120, 160, 3)).cuda()
    rects = [(0, 0, 64, 48), (40, 30, 80, 60), (96, 70, 64, 50)]
    base = hd.pack_candidates(det.detect_regions(image, rects))
    det.setScaleNMS(2)
    try:
        on = hd.pack_candidates(det.detect_regions(image, rects))
    finally:
        det.setScaleNMS(None)
    assert np.array_equal(on, filtered(base, 2)) and 0 < len(on) < len(base) and len(np.unique(on[:, 0])) == 3


def test_device_payloads_and_re_emission_under_another_dl(tiny):
    import torch
    model, det, hd, frames = tiny
    st = hd.stride
    batch = [synth.synthetic_frame(5 + i, 48, 64, 3) for i in range(2)]
    base = records(hd, batch)
    hd.set_scale_nms(1)
    try:
        want = filtered(base, 1).copy()
        want[:, 0] += 300
        cap = len(want) + 3
        pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
        d = torch.from_numpy(np.stack(batch)).cuda()
        det.detect_batch_device_out(d.data_ptr(), 2, 48, 64, 3, 300, pay.data_ptr(), cap)
        hd.check(hd.lib.pbd_synchronize(hd.h))
        got = pay.cpu().numpy()
        assert got[0] == len(want)                                      # word 0: the kept count
        assert np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), want)
        assert np.all(got[1 + len(want) * st:] == -7)
        # the resident result re-emitted under a second dl, and with the step off, without a new detect call
        hd.profile(True)
        for dl in (5, None):
            hd.set_scale_nms(dl)
            want = (base if dl is None else filtered(base, dl)).copy()
            want[:, 0] += 300
            pay = torch.full((1 + len(base) * st,), -7, dtype=torch.int32, device="cuda")
            det.argmin_device_out(300, pay.data_ptr(), len(base))
            hd.check(hd.lib.pbd_synchronize(hd.h))
            got = pay.cpu().numpy()
            assert got[0] == len(want) and np.array_equal(got[1:1 + len(want) * st].reshape(-1, st), want), dl
        prof = hd.profile_read()
        assert prof["k_scale_nms"][1] == 1 and prof["k_dt_rows"][1] == 0 and prof["k_conv"][1] == 0
    finally:
        hd.profile(False)
        hd.set_scale_nms(None)


def test_capacity_sees_only_the_kept_list(tiny):
    model, det, hd, frames = tiny
    small = detector.Handle(model, device=0, max_candidates=100)
    try:
        fr = [np.ascontiguousarray(frames[(48, 64)])]
        buf, n = np.zeros(100 * small.stride, np.int32), C.c_int()
        args = (small.h, 1, _lib.ptr_array(fr), 48, 64, 3, 64 * 3, buf.ctypes.data, 100, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4                      # off: 446 found, more than max_candidates
        small.set_scale_nms(0)
        assert small.lib.pbd_detect_batch(*args) == 0 and n.value == 22
        args = (small.h, 1, _lib.ptr_array(fr), 48, 64, 3, 64 * 3, buf.ctypes.data, 21, C.byref(n))
        assert small.lib.pbd_detect_batch(*args) == -4 and n.value == 21    # the caller's capacity below the kept count
    finally:
        small.close()


# ---- refusals and unaffected paths ---------------------------------------------------------------------------------------------
def test_refusals(tiny):
    model, det, hd, frames = tiny
    for dl in (-1, 256, 1 << 20):
        for enable in (0, 1):
            assert hd.lib.pbd_set_scale_nms(hd.h, enable, dl) == -1
            assert "scale NMS" in hd.lib.pbd_last_error(hd.h).decode()
    assert hd.lib.pbd_set_scale_nms(hd.h, 1, 255) == 0 and hd.lib.pbd_set_scale_nms(hd.h, 0, 0) == 0
    with pytest.raises(PbdError):
        detector.PartsBasedDetector(device=0).setScaleNMS(256)
    # level sharding, in either order of the two calls
    sh = detector.Handle(model, device=0)
    try:
        sh.set_level_shard(1, 2)
        assert sh.lib.pbd_set_scale_nms(sh.h, 1, 1) == -2
        assert sh.lib.pbd_set_scale_nms(sh.h, 0, 1) == 0                    # turning it off is always allowed
        sh.set_level_shard(0, 1)
        sh.set_scale_nms(1)
        assert sh.lib.pbd_set_level_shard(sh.h, 0, 2) == -2
        assert "scale NMS" in sh.lib.pbd_last_error(sh.h).decode()
        sh.set_scale_nms(None)
        sh.set_level_shard(0, 2)
    finally:
        sh.close()


def test_level_shards_merged_and_filtered_by_the_list_form(tiny):
    model, det, hd, frames = tiny
    im = frames[(48, 64)]
    want = with_scale_nms(hd, 2, [im])
    parts = []
    for rank in (0, 1):
        sh = detector.Handle(model, device=0)
        try:
            sh.set_level_shard(rank, 2)
            parts.append(records(sh, [im]))
        finally:
            sh.close()
    merged = topk.canonical_order(np.concatenate(parts))
    assert len(merged) == 446 and np.array_equal(hd.scale_nms(1, 2, merged), want)


def test_dp_argmin_detect_latent_and_examples_are_unaffected():
    model = M.synthetic_tiny_model(thresh=0.6)
    im = synth.synthetic_frame(31, 120, 150, 3)
    det = make(model, max_candidates=1 << 16)
    try:
        full = det.detect(im)
        best = max(full, key=lambda c: c.score())
        boxes = [[(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts]]

        def run():
            det.dp_.min(det.convolution_engine_.pdf(det.features_.pyramid(im)))
            staged = det.hd.pack_candidates(det.dp_.argmin(det.features_.scales()))
            rec, found = det.hd.detect_latent([im], boxes, 0.3)
            hdr, vals = det.examples(full[:20])
            return staged, rec.copy(), found.copy(), np.asarray(hdr).copy(), np.asarray(vals).copy()
        off = run()
        det.setScaleNMS(5)
        kept = det.detect(im)
        on = run()
        assert 0 < len(kept) < len(full)                            # the setting is on for detect ...
        assert len(off[0]) == len(full) >= 50                       # ... and DynamicProgram::argmin still lists every root
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        assert off[2].all()
        assert len(det.scaleNMS(full, 5)) == len(kept)              # the list form on the handle's own float records
    finally:
        det.hd.close()


# ---- the list form -------------------------------------------------------------------------------------------------------------
def device_scale_nms(hd, nframes, dl, rec, frame_offset=0, word0=None, out_cap=None):
    """pbd_scale_nms_device on a payload of the records; returns the output payload"""
    import torch
    st = hd.stride
    cap = max(len(rec), 1)
    pay = np.zeros(1 + cap * st, np.int32)
    pay[0] = len(rec) if word0 is None else word0
    pay[1:1 + rec.size] = rec.ravel()
    out_cap = cap if out_cap is None else out_cap
    d_in = torch.from_numpy(pay).cuda()
    d_out = torch.full((1 + max(out_cap, 1) * st,), -7, dtype=torch.int32, device="cuda")
    hd.scale_nms_device(nframes, dl, d_in.data_ptr(), cap, frame_offset, d_out.data_ptr(), out_cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return d_out.cpu().numpy()


@pytest.mark.parametrize("case", T.RECORD_CASES, ids=[c[0] for c in T.RECORD_CASES])
def test_list_host_and_device_forms(tiny, case):
    hd = tiny[2]
    name, rows, dl, kept = case
    st = hd.stride
    nframes = max(r[0] for r in rows) + 1
    for off in (0, 300):
        rec = T.record_list(rows, st, off)
        want = rec[kept]
        assert np.array_equal(S.filter_records(rec, dl, frame_offset=off, nframes=nframes), want)
        assert np.array_equal(hd.scale_nms(nframes, dl, rec, off), want)
        got = device_scale_nms(hd, nframes, dl, rec, off)
        assert got[0] == len(want) and np.array_equal(got[1:1 + want.size].reshape(-1, st), want)
        assert np.all(got[1 + want.size:] == -7)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257, 3000))
def test_list_sizes_in_place_and_own_records(tiny, n):
    model, det, hd, frames = tiny
    st = hd.stride
    rec = T.random_records(n, 7, 100 + n, st) if n else np.zeros((0, st), np.int32)
    for dl in (0, 1, 255):
        want = S.filter_records(rec, dl)
        buf = rec.copy() if n else np.zeros((1, st), np.int32)
        kept = C.c_int(-3)
        assert hd.lib.pbd_scale_nms(hd.h, 7, dl, buf.ctypes.data if n else None, n, 0, buf.ctypes.data if n else None, n,
                                    C.byref(kept)) == 0                                    # in place
        assert kept.value == len(want) and np.array_equal(buf[: len(want)], want)
        got = device_scale_nms(hd, 7, dl, rec)
        assert got[0] == len(want) and np.array_equal(got[1:1 + want.size].reshape(-1, st), want)
    if n == 3000:                                       # a float handle's own records: the detect-path form
        fr = [frames[(96, 128)]]
        base = records(hd, fr)
        for dl in (1, 5):
            assert np.array_equal(hd.scale_nms(1, dl, base), with_scale_nms(hd, dl, fr))


def test_list_word_0_conventions_and_refusals(tiny):
    hd = tiny[2]
    st = hd.stride
    rows = [(0, 3, 0, 3.0, 0, 0, 10, 10), (0, 3, 0, 1.0, 1, 1, 10, 10), (0, 3, 0, 2.0, 40, 40, 10, 10),
            (1, 3, 0, 5.0, 0, 0, 10, 10), (1, 3, 0, 4.0, 60, 0, 10, 10)]
    rec = T.record_list(rows, st)                   # kept: 0, 2, 3, 4
    for word0 in (-1, -4, 6):                       # a status, or more than the capacity: no complete list
        got = device_scale_nms(hd, 2, 1, rec, word0=word0)
        assert got[0] == -1 and np.all(got[1:] == -7)
    got = device_scale_nms(hd, 2, 0, rec, out_cap=3)   # the kept count may exceed the capacity: the first three are written
    assert got[0] == 4 and np.array_equal(got[1:1 + 3 * st].reshape(-1, st), rec[[0, 2, 3]])
    kept = C.c_int()
    out = np.zeros((5, st), np.int32)
    call = lambda nframes, dl, r, off=0: hd.lib.pbd_scale_nms(hd.h, nframes, dl, r.ctypes.data, len(r), off, out.ctypes.data, 5,
                                                              C.byref(kept))
    assert call(2, 0, rec) == 0 and kept.value == 4
    assert call(2, -1, rec) == -1 and call(2, 256, rec) == -1 and call(0, 1, rec) == -1
    assert call(1, 1, rec) == -1                    # a frame outside 0 .. nframes - 1
    assert call(2, 1, rec[::-1].copy()) == -1       # frames not ascending
    bad = rec.copy(); bad[1, 6] = 0
    assert call(2, 1, bad) == -1                    # nparts outside 1..max parts
    # the device form drops such records, and they are nobody's rival
    bad = rec.copy(); bad[0, 6] = 0                 # the best record of frame 0: record 1 now survives
    got = device_scale_nms(hd, 2, 0, bad)
    assert got[0] == 4 and np.array_equal(got[1:1 + 4 * st].reshape(-1, st), rec[[1, 2, 3, 4]])
    got = device_scale_nms(hd, 1, 0, rec)           # frame 1 is outside the call's one frame
    assert got[0] == 2 and np.array_equal(got[1:1 + 2 * st].reshape(-1, st), rec[[0, 2]])
    assert hd.lib.pbd_scale_nms_device(hd.h, 2, -1, 8, 1, 0, 8, 1) == -1
