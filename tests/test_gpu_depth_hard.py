"""The depth-consistency selects (k_dc_classify, k_dc_select_regs<64>, k_dc_select_regs<256>, k_dc_select_stream, k_dc_decide,
k_dc_emit) and the 3-D boxes (k_boxes3d) on the built hard depth images of tests/depth_hard_images.py, against the numpy
yardsticks consistency.filter_records and Candidate.boundingBox3D.  tests/test_depth_hard_cpu.py shows on the CPU that the cases
keep their promises and that a subtly wrong select changes what these tests compare.

Consistency runs with zfactor = 0, which makes a record's keep bit the bit equality of two medians; every comparison is of the
kept records' int32 words.  3-D boxes are compared by the float64 bit patterns of their six values.  No tolerance anywhere.

Wall times on an MI355X are in DESIGN.md sections 6c and 6f ("Built hard depth images")."""
import functools

import numpy as np
import pytest

import depth_hard_images as H
from test_gpu_boxes3d import assert_bits
from partsbaseddetector_amd import _lib, consistency, detector
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import Candidate

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
RTS = [_lib.REAL_F32, _lib.REAL_F64]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def two(request):
    """F32 and F64 handles of the 2-part model: part 1's parent is part 0"""
    model = M.synthetic_model(seed=5, pa=[0, 1], nmix=1, name="two")
    hs = {rt: detector.Handle(model, device=0, real_type=rt) for rt in RTS}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def person():
    hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=2)
    yield hd
    hd.close()


@functools.lru_cache(None)
def dc_cases():
    return H.consistency_cases()


def T_of(hd):
    return F32 if hd.dtype == np.float32 else F64


def to_device(img):
    import torch
    a = np.ascontiguousarray(img)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def run_dc_device(hd, img, rec, capacity=None, out_cap=None):
    """pbd_depth_consistency_device over one depth image: the whole output payload, every word past the kept records still -7"""
    import torch
    n = len(rec)
    capacity = n if capacity is None else capacity
    out_cap = n if out_cap is None else out_cap
    d_img = to_device(img)
    pay = torch.zeros(1 + capacity * hd.stride, dtype=torch.int32, device="cuda")
    pay[:1 + n * hd.stride] = torch.from_numpy(np.concatenate([[n], rec.ravel()]).astype(np.int32)).cuda()
    out = torch.full((1 + out_cap * hd.stride + 64,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hd.depth_consistency_device([(d_img.data_ptr(), img.shape[0], img.shape[1], img.strides[0])], _lib.DEPTH_CODE[np.dtype(img.dtype)],
                                0.0, pay.data_ptr(), capacity, 0, out.data_ptr(), out_cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return out.cpu().numpy()


def assert_payload(o, want, stride):
    assert o[0] == len(want)
    assert np.array_equal(o[1:1 + len(want) * stride].reshape(-1, stride), want)
    assert (o[1 + len(want) * stride:] == -7).all()               # nothing written past the kept records


# ---- depth consistency ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", ["u8", "u16", "f32", "f64"])
@pytest.mark.parametrize("rt", RTS)
def test_consistency_every_case(two, rt, code):
    """every built case of one depth code in one call: the three select kernels of that code and real type, every pass decisive"""
    hd = two[rt]
    T = T_of(hd)
    img, cases = dc_cases()[code]
    sel = [c for c in cases if T in c.keeps]
    rec = H.dc_records(sel, hd.stride)
    want = consistency.filter_records(hd.flat, rec, [img], 0.0, T)
    promised = np.array([c.keeps[T] for c in sel])
    assert np.array_equal(want, rec[promised])                    # the yardstick keeps the promises (also pinned without a GPU)
    assert 0 < len(want) < len(rec)                               # the group holds kept and dropped records
    got = hd.depth_consistency([img], rec, 0.0)
    if not np.array_equal(got, want):
        mine = {tuple(r) for r in got}
        wrong = [c.name for c, r in zip(sel, rec) if (tuple(r) in mine) != c.keeps[T]]
        pytest.fail(f"{len(wrong)} records decided wrongly: {wrong[:12]}")


@pytest.mark.parametrize("rt", RTS)
def test_consistency_emit_boundaries_host_and_device(two, rt):
    """kept records straddle the 256-record workgroups of k_dc_decide / k_dc_emit, and the workgroups keep different counts"""
    hd = two[rt]
    T = T_of(hd)
    img, cases = dc_cases()["f32"]
    rec, pattern = H.emit_list(H.probe_cases(cases, T), T, hd.stride)
    want = consistency.filter_records(hd.flat, rec, [img], 0.0, T)
    assert np.array_equal(want, rec[pattern]) and 0 < len(want) < len(rec)
    assert np.array_equal(hd.depth_consistency([img], rec, 0.0), want)
    assert_payload(run_dc_device(hd, img, rec), want, hd.stride)
    # a capacity above the count, and an output capacity below the kept count: word 0 is still the kept count
    o = run_dc_device(hd, img, rec, capacity=len(rec) + 300, out_cap=700)
    assert o[0] == len(want) and np.array_equal(o[1:1 + 700 * hd.stride].reshape(-1, hd.stride), want[:700])
    assert (o[1 + 700 * hd.stride:] == -7).all()


@pytest.mark.parametrize("rt", RTS)
def test_consistency_select_workgroups_take_a_second_median(two, rt):
    """each size class holds more medians than its select launch has workgroups (16 384 / 4096 / 1024): the grid-stride loops of
    k_dc_select_regs<64>, <256> and k_dc_select_stream re-enter dc_select with the LDS state of a median of other keys"""
    hd = two[rt]
    T = T_of(hd)
    img, cases = dc_cases()["f32"]
    rec, keep = H.reentry_list(cases, T, hd.stride)
    want = consistency.filter_records(hd.flat, rec, [img], 0.0, T)
    assert np.array_equal(want, rec[keep]) and 0 < len(want) < len(rec)
    got = hd.depth_consistency([img], rec, 0.0)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_consistency_second_classify_trip_host_and_device(person):
    """more than kDcMaxGrid * 256 (record, part) tasks: k_dc_classify's grid-stride loop makes a second trip.  Probe records
    (exact / off by one, all size classes) sit at every 97th position and densely across the 2^20-task boundary; every other
    record has all 26 boxes outside the image, so it has no median and keeps"""
    hd = person
    img, cases = dc_cases()["f32"]
    probes = H.probe_cases(cases, F32)
    n = 40400
    assert n * hd.max_parts > H.DC_MAX_GRID * H.DC_THREADS
    rec, which = H.long_list(probes, hd.stride, hd.max_parts, n, dense_from=40320)
    is_probe = which >= 0
    keep = np.ones(n, bool)
    kept_probes = consistency.filter_records(hd.flat, rec[is_probe], [img], 0.0, F32)
    keep[is_probe] = [probes[k].keeps[F32] for k in which[is_probe]]
    assert np.array_equal(kept_probes, rec[is_probe & keep])      # the yardstick on the probes; the rest keep by contract
    assert 100 < (~keep).sum() and (~keep[H.DC_MAX_GRID * H.DC_THREADS // hd.max_parts:]).any()
    want = rec[keep]
    got = hd.depth_consistency([img], rec, 0.0)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert_payload(run_dc_device(hd, img, rec), want, hd.stride)


# ---- 3-D boxes ---------------------------------------------------------------------------------------------------------------------
def cand(parts):
    parts = np.asarray(parts, np.int32).reshape(-1, 4)
    return Candidate(parts=parts, confidence=np.zeros(len(parts), np.float32), component=0)


def mirror(frames, cases):
    """Candidate.boundingBox3D per case; equal records (the long lists repeat a few) are computed once"""
    memo, out = {}, np.zeros((len(cases), 6))
    for i, c in enumerate(cases):
        k = (c.frame, tuple(map(tuple, c.parts)))
        if k not in memo:
            memo[k] = cand(c.parts).boundingBox3D(frames[c.frame].shape, frames[c.frame])
        out[i] = memo[k]
    return out


def test_boxes3d_sweeps(person):
    """the float32 step-in-ramp sweeps: the walk ends at nearly every row, so p[dmin] / p[dmax] come from nearly every pair of
    ranks; M = 2 .. 70 000, the copy path, the upsampling path, denormals, holes, several boxes, the NaN box"""
    frames, cases = H.boxes3d_sweeps()
    rec = H.b3_records(cases, person.stride)
    got = person.boxes3d(frames, [f.shape for f in frames], rec)
    assert_bits(got, mirror(frames, cases))
    assert np.isnan(got[:, 2]).sum() == 1                         # the one NaN box


@pytest.mark.parametrize("code", ["u8", "u16", "f64"])
def test_boxes3d_other_depth_codes(person, code):
    """k_boxes3d<kDepth8U>, <kDepth16U>, <kDepth64F>: a level with a one-count step; doubles that round to floats and to 0.0f"""
    frames, cases = H.boxes3d_coded(code)
    rec = H.b3_records(cases, person.stride)
    got = person.boxes3d(frames, [f.shape for f in frames], rec)
    want = mirror(frames, cases)
    assert_bits(got, want)
    assert len({tuple(r) for r in want[:, [2, 5]]}) >= 20         # the walk ended at many different places


def test_boxes3d_more_records_than_workgroups_host(person):
    """a workgroup computes record i and then record i + kB3MaxGrid: every kind after every other"""
    frames, cases = H.boxes3d_long_list(False)
    assert len(cases) > H.B3_MAX_GRID
    rec = H.b3_records(cases, person.stride)
    assert_bits(person.boxes3d(frames, [f.shape for f in frames], rec), mirror(frames, cases))


def test_boxes3d_more_records_than_workgroups_device(person):
    import torch
    frames, cases = H.boxes3d_long_list(True)
    n = len(cases)
    rec = H.b3_records(cases, person.stride)
    other = np.array([c.kind == "other" for c in cases])
    assert other.any() and (rec[other, 0] == -1).all()
    want = mirror(frames, [c if c.kind != "other" else c._replace(frame=0) for c in cases])
    want[other] = np.nan                                          # a record of another frame range: six NaNs
    d_frames = [to_device(f) for f in frames]
    descs = [(t.data_ptr(), f.shape[0], f.shape[1], f.strides[0]) for t, f in zip(d_frames, frames)]
    shapes = [f.shape for f in frames]

    def run(word0, capacity):
        pay = torch.zeros(1 + max(capacity, n) * person.stride, dtype=torch.int32, device="cuda")
        pay[:1 + n * person.stride] = torch.from_numpy(np.concatenate([[word0], rec.ravel()]).astype(np.int32)).cuda()
        out = torch.full((max(capacity, n) + 8, 6), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        person.boxes3d_device(descs, 5, shapes, pay.data_ptr(), capacity, 0, out.data_ptr())
        person.check(person.lib.pbd_synchronize(person.h))
        return out.cpu().numpy()

    o = run(n, n + 137)                                           # a capacity above the count
    assert_bits(o[:n], want)
    assert (o[n:] == 7.0).all()
    cap = H.B3_MAX_GRID + 252                                     # word 0 above the capacity: the first `capacity` records
    o = run(n, cap)
    assert_bits(o[:cap], want[:cap])
    assert (o[cap:] == 7.0).all()
