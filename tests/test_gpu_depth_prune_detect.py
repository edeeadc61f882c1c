"""Scale-depth pruning on the detect path (pbd_set_depth_prune + pbd_bind_depth*; Handle.set_depth_prune / bind_depth,
PartsBasedDetector.setDepthPrune).

The yardstick: the records of the same handle with the setting off, filtered by depthprune.filter_records -- the rule applied to
each record's own root rectangle.  Every comparison is of int32 record arrays: same content, same order, no tolerance.

Set-up: the tiny synthetic model with its threshold lowered until most root cells are hits; frames of 96x80 and 160x120 and one
of 200x176, whose level 0 alone has more root cells than one find block takes.  The depth images are built from the unpruned run's own
root rectangles: small blocks of pixels hold, at random, the depth one of the levels' box widths expects, or a hole -- so every
level keeps some of its roots and drops some, which the tests assert.
"""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import _lib, consistency, depthprune, detector, gridnms, synth
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu
THRESH = -0.5
FX, WIDTH, TOL = 500.0, 40.0, 0.02          # levels are a factor 2^(1/5) apart: bands of 2 % never overlap
CFG = (FX, WIDTH, TOL)
SMALL, MID, WIDE = (80, 96), (120, 160), (176, 200)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def frame(seed, shape):
    return synth.synthetic_frame(seed, shape[0], shape[1], 3)


def records(hd, frames, typed=None):
    """the raw records of one call: pbd_detect_typed (typed: a dtype), pbd_detect_batch for equal sizes, else pbd_detect_frames"""
    fr = [np.ascontiguousarray(f) for f in frames]
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    if typed is not None:
        im = np.ascontiguousarray(fr[0].astype(typed))
        hd.check(hd.lib.pbd_detect_typed(hd.h, im.ctypes.data, im.shape[0], im.shape[1], 3, im.strides[0], _lib.DEPTH_CODE[im.dtype],
                                         buf.ctypes.data, hd.max_candidates, C.byref(n)))
    elif len({f.shape for f in fr}) == 1:
        rows, cols, cn = fr[0].shape
        hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                         hd.max_candidates, C.byref(n)))
    else:
        descs = _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])
        hd.check(hd.lib.pbd_detect_frames(hd.h, len(fr), descs, 3, 0, buf.ctypes.data, hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def scene_depth(raw, f, shape, dtype, seed=0):
    """frame f's depth image from the root widths of its unpruned records: blocks of 5 x 5 pixels hold, at random, the depth one
    of the widths expects (rounded to the dtype), or 0"""
    widths = sorted({int(w) for w in raw[raw[:, 0] == f][:, 10]})
    vals = np.rint(np.array([FX * WIDTH / w for w in widths] + [0.0]))
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + 7919 * seed)
    idx = rng.integers(0, len(vals), (-(-shape[0] // 5), -(-shape[1] // 5)))
    return vals[np.kron(idx, np.ones((5, 5), np.int64))[: shape[0], : shape[1]]].astype(dtype)


def cuts_every_level(raw, want):
    """every (frame, level) with records keeps some and drops some"""
    key = lambda r: {(int(a), int(b)): n for (a, b), n in zip(*np.unique(r[:, [0, 2]], axis=0, return_counts=True))}
    all_, kept = key(raw), key(want)
    return len(all_) >= 10 and all(0 < kept.get(k, 0) < n for k, n in all_.items())


class Scene:
    """frames, their unpruned records on `hd`, depth images built from them, and the filtered list"""

    def __init__(self, hd, frames, dtype=np.uint16, typed=None, seed=0):
        self.frames = frames
        hd.set_depth_prune(None)
        self.raw = records(hd, frames, typed)
        self.depths = [scene_depth(self.raw, f, im.shape[:2], dtype, seed) for f, im in enumerate(frames)]
        self.want = depthprune.filter_records(self.raw, self.depths, *CFG)
        assert cuts_every_level(self.raw, self.want)


@pytest.fixture(scope="module")
def tiny():
    model = M.synthetic_tiny_model(thresh=THRESH)
    det = detector.PartsBasedDetector(device=0, max_batch=3)
    det.distributeModel(model)
    hd = det.hd
    sc = {"one": Scene(hd, [frame(61, SMALL)]),
          "wide": Scene(hd, [frame(63, WIDE)], np.float32),
          "batch": Scene(hd, [frame(61 + i, SMALL) for i in range(3)]),
          "mixed": Scene(hd, [frame(61, SMALL), frame(62, MID)], np.float64)}
    yield model, det, hd, sc
    hd.close()


def pruned(hd, scene, typed=None, depths=None):
    hd.set_depth_prune(*CFG)
    try:
        hd.bind_depth(scene.depths if depths is None else depths)
        return records(hd, scene.frames, typed)
    finally:
        hd.set_depth_prune(None)


@pytest.mark.parametrize("kind", ["one", "wide", "batch", "mixed"])
def test_pruned_detect_equals_the_filtered_unpruned_list(tiny, kind):
    """pbd_detect / pbd_detect_batch (3 frames) / pbd_detect_frames (2 sizes); `wide`: several find blocks per frame"""
    model, det, hd, sc = tiny
    s = sc[kind]
    assert len(s.raw) >= 1000 and 0 < len(s.want) < len(s.raw)
    if kind == "wide":
        assert (s.raw[:, 2] == 0).sum() > 1024 and len(s.raw) > 4 * 1024       # level 0 alone spans two find blocks
    got = pruned(hd, s)
    assert got.shape == s.want.shape and np.array_equal(got, s.want)
    keys = [tuple(r[[0, 2, 1, 4, 3]]) for r in got]
    assert keys == sorted(keys)


def test_typed_frames_and_every_depth_dtype(tiny):
    model, det, hd, sc = tiny
    s = Scene(hd, [frame(62, MID)], np.float32, typed=np.float32)           # pbd_detect_typed on a 32F image
    assert np.array_equal(pruned(hd, s, typed=np.float32), s.want)
    for dt in (np.uint16, np.float32, np.float64):
        depths = [scene_depth(s.raw, 0, MID, dt, seed=3)]
        want = depthprune.filter_records(s.raw, depths, *CFG)
        assert cuts_every_level(s.raw, want)
        assert np.array_equal(pruned(hd, s, typed=np.float32, depths=depths), want), dt
    # 8 bits cannot hold these depths: a sample is valid and wrong, or a hole (here, most are) -- only boxes that see nothing but
    # holes stay
    d8 = [np.where(s.depths[0] > 600, 200, 0).astype(np.uint8)]
    want = depthprune.filter_records(s.raw, d8, *CFG)
    assert 0 < len(want) < len(s.raw) // 4
    assert np.array_equal(pruned(hd, s, typed=np.float32, depths=d8), want)


def test_detector_surface_binds_when_pruning_is_on(tiny):
    model, det, hd, sc = tiny
    one, batch, mixed = sc["one"], sc["batch"], sc["mixed"]
    pack = hd.pack_candidates
    det.setDepthPrune(*CFG)
    try:
        assert np.array_equal(pack(det.detect(one.frames[0], one.depths[0])), one.want)
        assert np.array_equal(pack(det.detect(one.frames[0])), one.raw)                       # no depth: detect(im)
        assert np.array_equal(pack(det.detect_batch(batch.frames, depths=batch.depths)), batch.want)
        assert np.array_equal(pack(det.detect_batch(mixed.frames, depths=mixed.depths)), mixed.want)
        assert np.array_equal(pack(det.detect_frames(mixed.frames, depths=mixed.depths)), mixed.want)
        det.submit_batch(batch.frames, depths=batch.depths)                                    # _submit / _wait, and the setting
        assert hd.lib.pbd_set_depth_prune(hd.h, None) == -5                                    # is refused in flight
        assert "waited" in hd.lib.pbd_last_error(hd.h).decode()
        buf, n = det.wait_batch(raw=True)
        assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), batch.want)
    finally:
        det.setDepthPrune(None)
    assert np.array_equal(pack(det.detect(one.frames[0], one.depths[0])), one.raw)            # off: depth is ignored again


def test_device_out_regions_and_re_emission(tiny):
    import torch
    model, det, hd, sc = tiny
    st = hd.stride
    batch, mixed = sc["batch"], sc["mixed"]
    hd.set_depth_prune(*CFG)
    try:
        # pbd_detect_batch_device_out with device depth images that are regions of larger ones
        d_fr = torch.from_numpy(np.stack(batch.frames)).cuda()
        big = torch.zeros((3, SMALL[0] + 9, SMALL[1] + 13), dtype=torch.int16, device="cuda")
        for f in range(3):
            big[f, 4:4 + SMALL[0], 6:6 + SMALL[1]] = torch.from_numpy(batch.depths[f].view(np.int16)).cuda()
        torch.cuda.synchronize()
        pitch = (SMALL[1] + 13) * 2
        want = batch.want.copy()
        want[:, 0] += 100
        cap = len(want) + 5
        pay = torch.full((1 + cap * st,), -7, dtype=torch.int32, device="cuda")
        hd.bind_depth_device([(big[f, 4, 6:].data_ptr(), SMALL[0], SMALL[1], pitch) for f in range(3)], 2)
        det.detect_batch_device_out(d_fr.data_ptr(), 3, SMALL[0], SMALL[1], 3, 100, pay.data_ptr(), cap)
        hd.check(hd.lib.pbd_synchronize(hd.h))
        o = pay.cpu().numpy()
        assert o[0] == len(want) and np.array_equal(o[1:1 + len(want) * st].reshape(-1, st), want) and np.all(o[1 + len(want) * st:] == -7)
        # pbd_argmin_device_out re-emits the resident list: unpruned without a binding, then under a second binding
        raw = batch.raw.copy()
        raw[:, 0] += 100
        pay2 = torch.full((1 + len(raw) * st,), -7, dtype=torch.int32, device="cuda")
        det.argmin_device_out(100, pay2.data_ptr(), len(raw))
        hd.check(hd.lib.pbd_synchronize(hd.h))
        o = pay2.cpu().numpy()
        assert o[0] == len(raw) and np.array_equal(o[1:].reshape(-1, st), raw)
        other = [scene_depth(batch.raw, f, SMALL, np.float32, seed=5) for f in range(3)]
        want2 = depthprune.filter_records(batch.raw, other, *CFG)
        assert cuts_every_level(batch.raw, want2) and not np.array_equal(want2, batch.want)
        hd.bind_depth(other)
        pay2.fill_(-7)
        torch.cuda.synchronize()
        det.argmin_device_out(0, pay2.data_ptr(), len(raw))
        hd.check(hd.lib.pbd_synchronize(hd.h))
        o = pay2.cpu().numpy()
        assert o[0] == len(want2) and np.array_equal(o[1:1 + len(want2) * st].reshape(-1, st), want2)
    finally:
        hd.set_depth_prune(None)
    # detect_regions: two regions of one device image, each reading its own part of the image's depth map in place
    det.setDepthPrune(*CFG)
    try:
        canvas = np.zeros((MID[0] + 20, SMALL[1] + MID[1] + 30, 3), np.uint8)
        depth = np.zeros(canvas.shape[:2], np.float64)
        rects = [(5, 7, SMALL[1], SMALL[0]), (SMALL[1] + 20, 11, MID[1], MID[0])]
        for (x, y, w, h), im, d in zip(rects, mixed.frames, mixed.depths):
            canvas[y:y + h, x:x + w] = im
            depth[y:y + h, x:x + w] = d
        got = det.detect_regions(torch.from_numpy(canvas).cuda(), rects, depth=torch.from_numpy(depth).cuda())
        assert np.array_equal(hd.pack_candidates(got), mixed.want)
    finally:
        det.setDepthPrune(None)


@pytest.mark.parametrize("walk", [_lib.WALK_REFERENCE, _lib.WALK_ARGMAX])
def test_double_handle_and_both_walks(walk):
    hd = detector.Handle(M.synthetic_tiny_model(thresh=THRESH), device=0, max_batch=2, real_type=_lib.REAL_F64)
    try:
        hd.set_walk(walk)
        s = Scene(hd, [frame(61, SMALL), frame(62, MID)], np.float32)
        assert np.array_equal(pruned(hd, s), s.want)
    finally:
        hd.close()


def test_float_handle_argmax_walk(tiny):
    model, det, hd, sc = tiny
    hd.set_walk(_lib.WALK_ARGMAX)
    try:
        s = Scene(hd, sc["mixed"].frames)
        assert np.array_equal(pruned(hd, s), s.want)
    finally:
        hd.set_walk(_lib.WALK_REFERENCE)


@pytest.mark.parametrize("kind", ["batch", "mixed"])
def test_with_root_nms_the_maxima_are_taken_among_plausible_cells(tiny, kind):
    model, det, hd, sc = tiny
    s = sc[kind]
    hd.set_depth_prune(None)
    assert np.array_equal(records(hd, s.frames), s.raw)              # the unpruned run is resident: its rootv planes
    planes, shapes = {}, {}
    for f, im in enumerate(s.frames):
        pl = hd.plan(im.shape[0], im.shape[1])
        for l in range(pl["nlevels"]):
            r, c = int(pl["feat_rows"][l]), int(pl["feat_cols"][l])
            if r * c:
                shapes[(f, l)] = (r, c)
                planes[(f, l, 0)] = hd.get_stage(_lib.STAGE_ROOTV, f, l, r, c)[0]
    ok = depthprune.eligible_planes(s.raw, s.depths, *CFG, shapes=shapes)      # plausible and above the threshold
    kept = {k: gridnms.grid_nms_ref(p, 2, ok.get(k, np.zeros(p.shape, np.uint8))) for k, p in planes.items()}
    want = gridnms.filter_records(s.raw, lambda f, l, c: kept[(f, l, c)])
    plain = gridnms.filter_records(s.want, lambda f, l, c: gridnms.grid_nms_ref(planes[(f, l, c)], 2, planes[(f, l, c)] > np.float32(THRESH)))
    assert 20 <= len(want) < len(s.want) and not np.array_equal(want, plain)   # not root NMS first and the pruning after
    hd.set_root_nms(2)
    try:
        got = pruned(hd, s)
    finally:
        hd.set_root_nms(0)
    assert np.array_equal(got, want)


def test_with_set_nms_and_with_depth_consistency_chained(tiny):
    model, det, hd, sc = tiny
    for kind, shapes in (("batch", [SMALL] * 3), ("mixed", [SMALL, MID])):
        s = sc[kind]
        want = hd.suppress(shapes, 0.1, s.want)
        hd.set_nms(0.1)
        try:
            got = pruned(hd, s)
        finally:
            hd.set_nms(None)
        assert 1 <= len(want) < len(s.want) and np.array_equal(got, want), kind
    # detect(im, depth) with both settings and the suppression: prune at the roots -> consistency filter -> suppression
    s = sc["one"]
    im, depth = s.frames[0], s.depths[0].astype(np.float32)           # the same values: the same decisions
    mid = consistency.filter_records(hd.flat, s.want, [depth], 0.5, np.float32)
    want = hd.suppress([SMALL], 0.1, mid)
    assert 0 < len(mid) < len(s.want) and len(want) >= 1
    d2 = detector.PartsBasedDetector(device=0, nms=0.1)
    d2.setDepthPrune(*CFG)                                            # before distributeModel: kept across it
    d2.setDepthConsistency(0.5)
    d2.distributeModel(model)
    try:
        assert np.array_equal(d2.hd.pack_candidates(d2.detect(im, depth)), want)
        d2.setDepthConsistency(None)
        assert np.array_equal(d2.hd.pack_candidates(d2.detect(im, depth)), hd.suppress([SMALL], 0.1, s.want))
    finally:
        d2.hd.close()


def test_level_sharding(tiny):
    model, det, hd, sc = tiny
    s = sc["one"]
    sh = detector.Handle(model, device=0, max_batch=1)
    try:
        sh.set_level_shard(0, 2)
        raw = records(sh, s.frames)
        want = depthprune.filter_records(raw, s.depths, *CFG)
        levels = set(raw[:, 2].tolist())
        assert 0 < len(want) < len(raw) and 2 <= len(levels) < len(set(s.raw[:, 2].tolist()))
        assert np.array_equal(pruned(sh, s), want)
        assert np.array_equal(want, s.want[np.isin(s.want[:, 2], list(levels))])       # the rank's share of the unsharded result
    finally:
        sh.close()


def test_binding_is_consumed_and_off_equals_a_fresh_handle(tiny):
    model, det, hd, sc = tiny
    s = sc["one"]
    fresh = detector.Handle(model, device=0, max_batch=1)
    try:
        base = records(fresh, s.frames)
    finally:
        fresh.close()
    assert np.array_equal(base, s.raw)
    hd.set_depth_prune(*CFG)
    try:
        hd.bind_depth(s.depths)
        assert np.array_equal(records(hd, s.frames), s.want)
        assert np.array_equal(records(hd, s.frames), base)            # consumed: the second call has nothing bound
        hd.bind_depth(s.depths)
        hd.bind_depth(None)                                           # unbound again
        assert np.array_equal(records(hd, s.frames), base)
    finally:
        hd.set_depth_prune(None)
    hd.bind_depth(s.depths)                                           # bound but the setting off: dropped unused ...
    assert np.array_equal(records(hd, s.frames), base)
    hd.set_depth_prune(*CFG)
    try:
        assert np.array_equal(records(hd, s.frames), base)            # ... not kept for the next call
    finally:
        hd.set_depth_prune(None)


def test_mismatches_are_refused_and_leave_the_handle_usable(tiny):
    model, det, hd, sc = tiny
    one, batch, mixed = sc["one"], sc["batch"], sc["mixed"]
    hd.set_depth_prune(*CFG)
    try:
        for scene, depths, word in ((one, batch.depths[:2], "2 depth images"), (batch, batch.depths[:2], "2 depth images"),
                                    (one, [mixed.depths[1].astype(np.uint16)], "frame 0"),
                                    (batch, batch.depths[:2] + [np.zeros((SMALL[0], SMALL[1] + 1), np.uint16)], "frame 2"),
                                    (mixed, [mixed.depths[0], mixed.depths[0]], "frame 1")):
            hd.bind_depth(depths)
            with pytest.raises(PbdError) as e:
                records(hd, scene.frames)
            assert e.value.code == -1 and word in str(e.value)
            assert np.array_equal(records(hd, scene.frames), scene.raw)          # the binding is gone, the handle works
        # the resident result re-emitted under a binding of the wrong size
        import torch
        pay = torch.zeros(1 + len(mixed.raw) * hd.stride, dtype=torch.int32, device="cuda")
        hd.bind_depth(one.depths)
        with pytest.raises(PbdError) as e:
            det.argmin_device_out(0, pay.data_ptr(), len(mixed.raw))
        assert e.value.code == -1
        # refused images
        assert hd.lib.pbd_bind_depth(hd.h, 1, _lib.frame_array([(one.depths[0].ctypes.data, 80, 96, 96)]), 2) == -1
        assert hd.lib.pbd_bind_depth(hd.h, 1, _lib.frame_array([(one.depths[0].ctypes.data, 80, 96, 192)]), 3) == -1
        assert hd.lib.pbd_bind_depth(hd.h, -1, None, 2) == -1 and hd.lib.pbd_bind_depth(hd.h, 1, None, 2) == -1
        assert hd.lib.pbd_bind_depth_device(hd.h, 1, _lib.frame_array([(pay.data_ptr() + 1, 8, 8, 16)]), 2) == -1
        for cfg in ((0.0, 1.0, 0.1), (1.0, -1.0, 0.1), (1.0, 1.0, -0.1), (np.nan, 1.0, 0.1), (1.0, np.inf, 0.1), (1.0, 1.0, np.nan)):
            assert hd.lib.pbd_set_depth_prune(hd.h, hd._prune_cfg(*cfg)) == -1
        hd.bind_depth(one.depths)
        assert np.array_equal(records(hd, one.frames), one.want)                 # a refused cfg left the setting as it was
    finally:
        hd.set_depth_prune(None)


def test_dp_argmin_and_detect_latent_are_unaffected(tiny):
    model, det, hd, sc = tiny
    s = sc["one"]
    im = s.frames[0]
    best = max(hd.unpack_candidates(s.raw.ravel(), len(s.raw)), key=lambda c: c.score())
    boxes = [[(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in best.parts]]

    def run():
        det.dp_.min(det.convolution_engine_.pdf(det.features_.pyramid(im)))
        hd.bind_depth(s.depths)                                       # a binding DynamicProgram::argmin must not use
        staged = hd.pack_candidates(det.dp_.argmin(det.features_.scales()))
        hd.bind_depth(s.depths)
        rec, found = hd.detect_latent([im], boxes, 0.3)
        hd.bind_depth(None)
        return staged, rec.copy(), found.copy()
    off = run()
    hd.set_depth_prune(*CFG)
    try:
        on = run()
    finally:
        hd.set_depth_prune(None)
    assert len(off[0]) == len(s.raw) and off[2].all()               # DynamicProgram::argmin still lists every root
    for a, b in zip(off, on):
        assert np.array_equal(a, b)


def test_detector_pool_forwards_the_setting_and_binds_per_lane(tiny):
    model, det, hd, sc = tiny
    s = sc["batch"]
    pool = detector.DetectorPool(model, n=2, device=0, max_batch=3)
    try:
        pool.setDepthPrune(*CFG)
        pool.submit_batch(s.frames, depths=s.depths)
        pool.submit_batch(s.frames)                                   # the other lane, nothing bound
        for want in (s.want, s.raw):
            buf, n = pool.wait_batch(raw=True)
            assert np.array_equal(np.array(buf[: n * hd.stride]).reshape(n, -1), want)
    finally:
        pool.close()
