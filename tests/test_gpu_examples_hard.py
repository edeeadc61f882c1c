"""k_ex_walk and k_ex_gather (csrc/pbd_kernels_examples.hip) on the built records of tests/latent_hard_cases.py, host and device
forms against examples.examples_of_records on the oracle's maps: filters of 1, 3, 5, 6, 9 and 12 cells at the corners, edges and
centre of the first, middle and last level; more (record, part) pairs than the gather's grid holds; and every device-side check
of a record in a mixed-size plan with a frame offset, with three count words.

Every comparison is of integers or of BIT PATTERNS.  There is no tolerance anywhere in this file.

k_ex_walk's own grid-stride loop (more than 8192 x 128 records, tens of GB of values) is not reached here."""
import numpy as np
import pytest

import latent_hard_cases as L
from partsbaseddetector_amd import _lib, detector
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError

from test_gpu_examples import records

pytestmark = pytest.mark.gpu

REAL = {np.float32: _lib.REAL_F32, np.float64: _lib.REAL_F64}
SENTINEL = -7


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def device_examples(hd, rec, count, capacity, rows, frame_offset=0):
    """pbd_examples_device of a payload holding `rec` under the count word `count`, into buffers of `rows` examples filled with
    SENTINEL: (hdr, values) as numpy arrays"""
    import torch
    hw, vw = hd.example_stride()
    pay = torch.zeros(1 + max(len(rec), 1) * hd.stride, dtype=torch.int32, device="cuda")
    pay[0] = count
    if len(rec):
        pay[1:1 + rec.size] = torch.from_numpy(np.ascontiguousarray(rec).ravel()).cuda()
    d_hdr = torch.full((rows, hw), SENTINEL, dtype=torch.int32, device="cuda")
    d_val = torch.full((rows, vw), SENTINEL, dtype=torch.float32 if hd.dtype == np.float32 else torch.float64, device="cuda")
    hd.examples_device(pay.data_ptr(), capacity, frame_offset, d_hdr.data_ptr(), d_val.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return d_hdr.cpu().numpy(), d_val.cpu().numpy()


def assert_examples(hdr, vals, want_h, want_v):
    assert np.array_equal(hdr, want_h)
    for i in range(len(want_h)):
        n = int(want_h[i, 3])
        assert vals[i, :n].tobytes() == want_v[i, :n].tobytes(), i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(L.SIZES))
def test_built_records_of_every_filter_size(name, dtype):
    model = L.sizes_model(name)
    flat = model.flatten()
    fm = L.frame_maps("sizes", name, np.dtype(dtype).name)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 16)
    try:
        records(hd, [L.sizes_frame()])
        rec = L.record_rows(hd.stride, L.built_entries(flat, L.level_shapes(fm)))
        want_h, want_v = E.examples_of_records(flat, [fm], rec, 0, dtype)
        assert_examples(*hd.examples(rec), want_h, want_v)
        hdr, vals = device_examples(hd, rec, len(rec), len(rec), len(rec) + 2)
        assert_examples(hdr[:len(rec)], vals[:len(rec)], want_h, want_v)
        assert np.all(hdr[len(rec):] == SENTINEL) and np.all(vals[len(rec):] == SENTINEL)
    finally:
        hd.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_beyond_its_grid(dtype):
    """1300 records of 26 parts: more (record, part) pairs than the 8192 blocks x 4 waves k_ex_gather starts with, so its
    stride loop goes round a second time"""
    model = M.synthetic_person_model(thresh=L.LOW)
    flat = model.flatten()
    fm = L.frame_maps("person", "120x160", np.dtype(dtype).name)
    hd = detector.Handle(model, device=0, real_type=REAL[dtype], max_candidates=1 << 14)
    try:
        records(hd, [L.person_frame()])
        _, pos = L.seeded_positions(L.level_shapes(fm), L.GATHER_RECORDS)
        rec = L.record_rows(hd.stride, [(0, 0, l, x, y) for (l, x, y) in pos])
        assert len(rec) * hd.max_parts > L.GATHER_WAVES * L.GATHER_GRID
        want_h, want_v = E.examples_of_records(flat, [fm], rec, 0, dtype)
        assert_examples(*hd.examples(rec), want_h, want_v)
    finally:
        hd.close()


@pytest.fixture(scope="module")
def bad_plan():
    """the handle after a mixed-size detect of the three frames, the records (good and bad interleaved), the reason of each bad
    one, and the yardstick's example of each good one under its index in the list"""
    model = L.bad_model()
    flat = model.flatten()
    frames = L.bad_frames()
    hd = detector.Handle(model, device=0, max_batch=4, max_candidates=1 << 18)
    records(hd, frames)
    maps = [E.FrameMaps(flat, f) for f in frames]
    shapes = [L.level_shapes(fm) for fm in maps]
    entries = L.bad_entries([len(s) for s in shapes], shapes, flat.ncomponents)
    rec = L.record_rows(hd.stride, [e for e, _ in entries], L.BAD_OFFSET)
    reasons = [r for _, r in entries]
    want = {}
    for i, ((f, c, l, x, y), reason) in enumerate(entries):
        if reason is None:
            want[i] = E.example(flat, maps[f].feats[l], c, maps[f].placement(l, c, x, y), i)
    yield hd, rec, reasons, want
    hd.close()


def assert_bad_plan_rows(hdr, vals, rec, reasons, want, upto):
    """rows [0, upto) are written (a bad record: {i, component, -1, 0 ...} and an untouched value row; a good one: the
    yardstick's), the rows from `upto` on are untouched"""
    for i in range(upto):
        if reasons[i] is None:
            want_h, want_v = want[i]
            assert np.array_equal(hdr[i], want_h), i
            n = int(want_h[3])
            assert vals[i, :n].tobytes() == want_v[:n].tobytes(), i
        else:
            assert list(hdr[i, :3]) == [i, rec[i, 1], -1] and not hdr[i, 3:].any(), (i, reasons[i])
            assert np.all(vals[i] == SENTINEL), (i, reasons[i])
    assert np.all(hdr[upto:] == SENTINEL) and np.all(vals[upto:] == SENTINEL)


def test_bad_records_device_form(bad_plan):
    hd, rec, reasons, want = bad_plan
    n = len(rec)
    assert sum(r is not None for r in reasons) == 8
    hdr, vals = device_examples(hd, rec, n, n, n + 3, L.BAD_OFFSET)
    assert_bad_plan_rows(hdr, vals, rec, reasons, want, n)
    # a count word above the capacity is clamped to it: the rows past the capacity are untouched
    cap = n - 4
    assert reasons[cap - 1] is not None or reasons[cap - 2] is not None
    hdr, vals = device_examples(hd, rec, n + 1000, cap, n + 3, L.BAD_OFFSET)
    assert_bad_plan_rows(hdr, vals, rec, reasons, want, cap)
    for count in (-1, 0):
        hdr, vals = device_examples(hd, rec, count, n, n + 3, L.BAD_OFFSET)
        assert_bad_plan_rows(hdr, vals, rec, reasons, want, 0)


def test_bad_records_host_form(bad_plan):
    hd, rec, reasons, want = bad_plan
    good = [i for i, r in enumerate(reasons) if r is None]
    hdr, vals = hd.examples(rec[good], L.BAD_OFFSET)
    for k, i in enumerate(good):
        want_h, want_v = want[i]
        assert np.array_equal(hdr[k, 1:], want_h[1:]) and hdr[k, 0] == k
        n = int(want_h[3])
        assert vals[k, :n].tobytes() == want_v[:n].tobytes(), i
    for i, reason in enumerate(reasons):
        if reason is None:
            continue
        with pytest.raises(PbdError) as e:                     # behind its good neighbour: record 1 of the two
            hd.examples(rec[i - 1:i + 1], L.BAD_OFFSET)
        assert e.value.code == -1 and "record 1:" in str(e.value), reason
