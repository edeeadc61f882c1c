"""k_latent_mask and k_latent_best (csrc/pbd_kernels_examples.hip) on the built cases of tests/latent_hard_cases.py: after
pbd_detect_latent every level's masked responses, root scores and root mixtures are read back with pbd_get_stage and compared with
the yardstick (examples.mask_responses of the oracle's responses, the oracle's dynamic program on them), the record and `found`
with the first maximum in (level, component, y, x) order, and the positive's example with examples.example of the yardstick's
placement.  The conditions the cases are built for are asserted without a GPU in tests/test_latent_hard_cpu.py.

Every comparison is of BIT PATTERNS (planes, scores, values) or of integers.  There is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import latent_hard_cases as L
from partsbaseddetector_amd import _lib, detector, synth
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

from test_gpu_examples import records

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
WALK = {"reference": _lib.WALK_REFERENCE, "argmax": _lib.WALK_ARGMAX}
STAGES = (_lib.STAGE_FEATURES, _lib.STAGE_RESPONSES, _lib.STAGE_ROOTV, _lib.STAGE_ROOTI)
CASES = [(name, walk) for name in L.LATENT_CASES for walk in (("reference", "argmax") if name in L.BOTH_WALKS else ("reference",))]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_record(r, f, st, walk):
    """one record of pbd_detect_latent == the yardstick's best root, its score in float and its walked part boxes"""
    assert tuple(int(v) for v in r[:5]) == (f, st["component"], st["level"], st["root_x"], st["root_y"]), (f, r[:5])
    assert r[5:6].view(np.float32)[0].tobytes() == np.float32(st["score"]).tobytes()
    want = st["parts"][walk]
    assert r[6] == len(want) and np.array_equal(r[8:8 + 4 * r[6]].reshape(-1, 4), want)


def first_maximum(planes):
    """(level, component, x, y, value) of the first maximum of [level] (NC, H, W) planes in (level, component, y, x) order"""
    best = None
    for lvl, rv in enumerate(planes):
        i = int(np.argmax(rv))
        if best is None or rv.flat[i] > best[4]:
            c, y, x = np.unravel_index(i, rv.shape)
            best = (lvl, int(c), int(x), int(y), rv.flat[i])
    return best


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,walk", CASES)
def test_case_stage_by_stage(name, walk, dtype):
    case = L.latent_case(name)
    want = L.latent_yardstick(name, np.dtype(dtype).name)
    flat = case.model.flatten()
    hd = detector.Handle(case.model, device=0, real_type=REAL[dtype], max_batch=len(case.frames), max_candidates=1 << 12)
    try:
        hd.set_walk(WALK[walk])
        rec, found = hd.detect_latent(case.frames, case.boxes, case.overlap, case.mixtures)
        for f, st in enumerate(want):
            for lvl in range(len(st["feats"])):
                _, rows, cols = st["rootv"][lvl].shape
                assert same(hd.get_stage(_lib.STAGE_FEATURES, f, lvl, rows, cols), st["feats"][lvl]), (f, lvl)
                assert same(hd.get_stage(_lib.STAGE_RESPONSES, f, lvl, rows, cols), st["resp"][lvl]), (f, lvl)
                assert same(hd.get_stage(_lib.STAGE_ROOTV, f, lvl, rows, cols), st["rootv"][lvl]), (f, lvl)
                assert same(hd.get_stage(_lib.STAGE_ROOTI, f, lvl, rows, cols), st["rooti"][lvl]), (f, lvl)
            with pytest.raises(PbdError) as e:                     # a level of another frame's deeper pyramid is not this frame's
                hd.get_stage(_lib.STAGE_ROOTV, f, len(st["feats"]), 1, 1)
            assert e.value.code == -1
            check_record(rec[f], f, st, walk)
            assert bool(found[f]) == st["found"]
        hdr, vals = hd.examples(rec)
        for f, st in enumerate(want):
            want_h, want_v = E.example(flat, st["feats"][st["level"]], st["component"], st["placement"][walk], f, dtype)
            assert np.array_equal(hdr[f], want_h)
            n = int(want_h[3])
            assert vals[f, :n].tobytes() == want_v[:n].tobytes(), f
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_keep_all_is_a_plain_detection_of_the_unique_model(dtype):
    """overlap -1 masks nothing: every stage and the record are those of a handle made from unique_model(model) after a plain
    detect of the frame"""
    case = L.latent_case("keep_all")
    hd = detector.Handle(case.model, device=0, real_type=REAL[dtype], max_candidates=1 << 12)
    plain = detector.Handle(E.unique_model(case.model), device=0, real_type=REAL[dtype], max_candidates=1 << 16)
    try:
        rec, found = hd.detect_latent(case.frames, case.boxes, case.overlap)
        every = records(plain, case.frames)
        p = hd.plan(*case.frames[0].shape[:2])
        rootv = []
        for lvl in range(p["nlevels"]):
            shape = int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl])
            for s in STAGES:
                assert same(hd.get_stage(s, 0, lvl, *shape), plain.get_stage(s, 0, lvl, *shape)), (lvl, s)
            rootv.append(plain.get_stage(_lib.STAGE_ROOTV, 0, lvl, *shape))
        lvl, c, x, y, _ = first_maximum(rootv)
        row, = [r for r in every if tuple(r[1:5]) == (c, lvl, x, y)]
        assert np.array_equal(rec[0], row) and found[0] == 1
    finally:
        plain.close()
        hd.close()


def check_masked_levels(hd, plain, model, im, boxes, overlap, dtype):
    """every level's masked responses of hd == where(keep, the plain unique-model handle's unmasked responses, -1e10) with keep
    from examples.part_rects / overlap_passes.  Returns the number of kept values and hd's ROOTV planes."""
    uflat = E.unique_model(model).flatten()
    p = hd.plan(*im.shape[:2])
    kept, rootv = 0, []
    for lvl in range(p["nlevels"]):
        rows, cols = int(p["feat_rows"][lvl]), int(p["feat_cols"][lvl])
        want = plain.get_stage(_lib.STAGE_RESPONSES, 0, lvl, rows, cols)
        ys, xs = np.mgrid[0:rows, 0:cols]
        keep = {}
        for gp in range(uflat.part_offset[0], uflat.part_offset[-1]):
            part = gp - int(uflat.part_offset[np.searchsorted(uflat.part_offset, gp, side="right") - 1])
            for gm in range(uflat.mix_offset[gp], uflat.mix_offset[gp + 1]):
                key = (part, int(uflat.filter_ksize[gm]))
                if key not in keep:
                    keep[key] = E.overlap_passes(E.part_rects(xs, ys, key[1], p["scales"][lvl], dtype), boxes[part], L.widened(overlap))
                want[gm][~keep[key]] = dtype(E.MASKED)
        assert same(hd.get_stage(_lib.STAGE_RESPONSES, 0, lvl, rows, cols), want), lvl
        kept += int((want != dtype(E.MASKED)).sum())
        rootv.append(hd.get_stage(_lib.STAGE_ROOTV, 0, lvl, rows, cols))
    return kept, rootv


def check_masked(hd, plain, model, im, boxes, overlap, dtype):
    """plain: a handle of unique_model(model) whose resident result is a plain detect of im"""
    rec, found = hd.detect_latent([im], [boxes], overlap)
    kept, rootv = check_masked_levels(hd, plain, model, im, boxes, overlap, dtype)
    assert kept > 0 and found[0] == 1
    lvl, c, x, y, v = first_maximum(rootv)
    assert tuple(int(t) for t in rec[0, :5]) == (0, c, lvl, x, y)
    assert rec[0, 5:6].view(np.float32)[0].tobytes() == np.float32(v).tobytes()


def test_mask_beyond_the_grid_cap():
    """One 480 x 640 frame of the person model: more response values than the 65536 x 256 threads of k_latent_mask's capped grid,
    so its grid-stride loop goes round a second time.  The oracle's dynamic program is not run on this frame."""
    model = M.synthetic_person_model(thresh=L.LOW)
    im = synth.synthetic_frame(1, 480, 640)
    hd = detector.Handle(model, device=0, max_candidates=1 << 12)
    plain = detector.Handle(E.unique_model(M.synthetic_person_model()), device=0, max_candidates=1 << 12)
    try:
        p = hd.plan(480, 640)
        cells = int((p["feat_rows"].astype(np.int64) * p["feat_cols"]).sum())
        assert cells * int(hd.flat.mix_offset[-1]) > L.MASK_GRID * L.MASK_THREADS
        every = records(plain, [im])           # at the model's own threshold: some tens of records, the best gives the boxes
        best = max(plain.unpack_candidates(every.ravel(), len(every)), key=lambda c: c.score())
        boxes = [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts]
        check_masked(hd, plain, model, im, boxes, np.float32(0.5), np.float32)
    finally:
        plain.close()
        hd.close()


@pytest.mark.parametrize("mode,dtype,sizes", [(_lib.CONV_FMA, np.float32, "9_12_5"), (_lib.CONV_MFMA, np.float32, "5"),
                                              (_lib.CONV_MFMA_F64, np.float64, "9_12_5")])
def test_mask_in_other_convolution_modes(mode, dtype, sizes):
    """the inexact modes have no CPU yardstick for the responses, so the mask is checked on the same mode's own unmasked
    responses: a handle of unique_model(model) after a plain detect of the frame.  PBD_CONV_MFMA takes 5 x 5 filters only, so it
    runs the sizes model that has no others."""
    case = L.sizes_case(sizes)
    hd = detector.Handle(case.model, device=0, real_type=REAL[dtype], conv_mode=mode, max_candidates=1 << 12)
    plain = detector.Handle(E.unique_model(case.model), device=0, real_type=REAL[dtype], conv_mode=mode, max_candidates=1 << 16)
    try:
        records(plain, case.frames)
        check_masked(hd, plain, case.model, case.frames[0], case.boxes[0], case.overlap, dtype)
    finally:
        plain.close()
        hd.close()


def test_stage_refusals():
    """pbd_get_stage reads a latent result and nothing else does; a refusal is reported on the handle; after a model update, a
    warp and before any call it refuses as it did"""
    import torch
    case = L.latent_case("half")
    hd = detector.Handle(case.model, device=0, max_candidates=1 << 12)
    try:
        with pytest.raises(PbdError) as e:
            hd.get_stage(_lib.STAGE_RESPONSES, 0, 0, 16, 22)
        assert e.value.code == -5
        hd.detect_latent(case.frames, case.boxes, case.overlap)
        got = hd.get_stage(_lib.STAGE_RESPONSES, 0, 0, 16, 22)
        assert got.shape[0] == int(hd.flat.mix_offset[-1])
        pay = torch.zeros(1 + 16 * hd.stride, dtype=torch.int32, device="cuda")
        assert hd.lib.pbd_argmin_device_out(hd.h, 0, pay.data_ptr(), 16) == -5
        scales = np.ones(_lib.MAX_LEVELS, np.float32)
        buf, n = np.zeros(16 * hd.stride, np.int32), C.c_int()
        assert hd.lib.pbd_dp_argmin(hd.h, _lib.ptr(scales, C.c_float), buf.ctypes.data, 16, C.byref(n)) == -5
        for args, code, text in (((_lib.STAGE_ROOTV, 1, 0, 16, 22), -1, "out of range"), ((_lib.STAGE_ROOTV, 0, -1, 16, 22), -1, "out of range"),
                                 ((7, 0, 0, 16, 22), -1, "unknown stage"), ((_lib.STAGE_ROOTI, 0, 0, 8, 22), -1, "destination holds")):
            dst = np.zeros((hd.flat.ncomponents, args[3], args[4]), np.int32)
            assert hd.lib.pbd_get_stage(hd.h, args[0], args[1], args[2], dst.ctypes.data, dst.nbytes) == code
            assert text in hd.lib.pbd_last_error(hd.h).decode()
        assert same(hd.get_stage(_lib.STAGE_RESPONSES, 0, 0, 16, 22), got)      # a refused call leaves the result readable
        hd.set_model_vector(hd.model_vector())
        for s in STAGES:
            with pytest.raises(PbdError) as e:
                hd.get_stage(s, 0, 0, 16, 22)
            assert e.value.code == -5
        hd.detect_latent(case.frames, case.boxes, case.overlap)
        assert same(hd.get_stage(_lib.STAGE_RESPONSES, 0, 0, 16, 22), got)
        hd.warp_positives(case.frames, np.array([[0, 8, 8, 47, 47]], np.int32))
        with pytest.raises(PbdError) as e:
            hd.get_stage(_lib.STAGE_FEATURES, 0, 0, 16, 22)
        assert e.value.code == -5
    finally:
        hd.close()
