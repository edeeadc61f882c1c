"""The layer that keeps more than one batch in flight, on hard orders: the two-slot pbd_detect_batch_submit /
pbd_detect_batch_device_submit / pbd_detect_batch_wait state machine of a handle, and detector.DetectorPool over three handles.

Every expected list is the CPU oracle's (tests/pipeline_cases.py: oracle.detect per frame, float, laid out as records in the
order of pbd_detect_batch; with the post-processing stage on, the Python mirror of Candidate.sort + nonMaximaSuppression on
those records).  Records are compared as int32 arrays: same content, same order, no tolerance.  The C entry points are called
through ctypes so that status codes, *ncand and the words behind the delivered records are seen as the ABI leaves them.

Nothing here provokes a GPU fault: every failure is a host-side refusal or PBD_ERR_CAPACITY on a completed batch.
"""
import ctypes as C

import numpy as np
import pytest

import pipeline_cases as PC
from partsbaseddetector_amd import _lib, detector
from partsbaseddetector_amd.detector import PbdError

pytestmark = pytest.mark.gpu
ST = PC.stride()
CAP = PC.MAX_CANDIDATES
FILL = -7                       # what the result buffers hold before a wait: nothing may be written behind the delivered records
OK, INVALID, CAPACITY, STATE = 0, -1, -4, -5


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch's HIP runtime is initialised before this module creates its first handle (as the suite's earlier modules do)"""
    import torch
    torch.cuda.init()


def make(max_candidates=CAP, nms=None):
    det = detector.PartsBasedDetector(device=0, max_batch=PC.MAX_BATCH, max_candidates=max_candidates)
    det.distributeModel(PC.model())
    assert det.hd.stride == ST
    if nms is not None:
        det.hd.set_nms(nms)
    return det


class Driver:
    """one handle, driven through the C entry points; keeps the device tensors of device-form submits alive until their wait"""

    def __init__(self, det):
        self.det, self.hd, self.lib, self.h = det, det.hd, det.hd.lib, det.hd.h
        self.dev = []

    def submit_host(self, frames, pad=0, zero_after=False):
        """frames: arrays this call copies into buffers of its own, rows `pad` bytes longer than the pixels (the padding holds
        255); zero_after: everything is overwritten with 0 as soon as submit() has returned"""
        rows, cols, cn = frames[0].shape
        own = []
        for f in frames:
            a = np.full((rows, cols * cn + pad), 255, np.uint8)
            a[:, :cols * cn] = f.reshape(rows, cols * cn)
            own.append(a)
        rc = self.lib.pbd_detect_batch_submit(self.h, len(own), _lib.ptr_array(own), rows, cols, cn, cols * cn + pad)
        if zero_after:
            for a in own:
                a[:] = 0
        return rc

    def submit_device(self, frames):
        import torch
        rows, cols, cn = frames[0].shape
        d = torch.from_numpy(np.stack(frames)).cuda()
        rc = self.lib.pbd_detect_batch_device_submit(self.h, len(frames), d.data_ptr(), rows, cols, cn)
        if rc == OK:
            self.dev.append(d)                      # untouched until the matching wait returns (include/pbd.h)
        return rc

    def submit(self, name, form):
        fr = PC.batch_frames(name)
        return self.submit_host(fr) if form == "host" else self.submit_device(fr)

    def wait(self, capacity=CAP):
        """(status, *ncand, delivered records) -- after checking that nothing was written behind the delivered records"""
        buf = np.full(capacity * ST + 3, FILL, np.int32)
        n = C.c_int(-99)
        rc = self.lib.pbd_detect_batch_wait(self.h, buf.ctypes.data, capacity, C.byref(n))
        if rc != STATE:
            assert 0 <= n.value <= capacity, n.value
            assert np.all(buf[n.value * ST:] == FILL)
            return rc, n.value, buf[: n.value * ST].reshape(n.value, ST)
        return rc, n.value, None

    def sync_batch(self, name, capacity=CAP):
        fr = [np.ascontiguousarray(f) for f in PC.batch_frames(name)]
        rows, cols, cn = fr[0].shape
        buf = np.full(capacity * ST, FILL, np.int32)
        n = C.c_int(-99)
        rc = self.lib.pbd_detect_batch(self.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data, capacity,
                                       C.byref(n))
        return rc, n.value, buf

    def expect(self, name, capacity=CAP):
        """the next wait returns batch `name`'s oracle list, whole"""
        rc, n, rec = self.wait(capacity)
        want = PC.batch_records(name)
        assert rc == OK, (name, rc, self.lib.pbd_last_error(self.h).decode())
        assert n == len(want), (name, n, len(want))
        assert np.array_equal(rec, want), name

    def close(self):
        self.dev.clear()
        self.hd.close()


def test_growth_in_flight_and_reuse_of_grown_slots():
    """A second batch that needs every workspace larger (3 frames of 120x160 after 1 of 64x80; a list longer than the speculative
    read-back covers) is submitted while the first is still running; then the reverse on a fresh handle; then the first handle
    goes on with the other batches, host and device forms alternating so that both slots see both, in another order."""
    a = Driver(make())
    assert a.submit("small", "host") == OK          # slot 0
    assert a.submit("large", "host") == OK          # slot 1: grows pinned staging, frames, workspaces, payload mirror
    a.expect("small")
    a.expect("large")
    b = Driver(make())                              # reversed, on a fresh handle: the first wait's list outruns the guess while
    assert b.submit("large", "host") == OK          # the second batch's kernels hold the compute stream
    assert b.submit("small", "host") == OK
    b.expect("large")
    b.expect("small")
    b.close()
    assert a.submit("blank", "device") == OK        # slot 0, device form
    assert a.submit("pair", "host") == OK           # slot 1, host form, another frame size
    a.expect("blank")
    a.expect("pair")
    # the same four again, another order, one batch ahead of the wait; slot 0: device, host -- slot 1: device, device
    assert a.submit("large", "device") == OK
    assert a.submit("blank", "device") == OK
    a.expect("large")
    assert a.submit("pair", "host") == OK
    a.expect("blank")
    assert a.submit("small", "device") == OK
    a.expect("pair")
    a.expect("small")
    assert a.wait()[0] == STATE
    a.close()


def test_frames_are_copied_before_submit_returns():
    """pbd_detect_batch_submit on arrays the test owns, rows 13 bytes longer than the pixels, zeroed as soon as the call is
    back; a second batch likewise.  Both waits deliver the lists of the ORIGINAL pixels."""
    d = Driver(make())
    assert d.submit_host(PC.batch_frames("large"), pad=13, zero_after=True) == OK
    assert d.submit_host(PC.batch_frames("pair"), pad=13, zero_after=True) == OK
    d.expect("large")
    d.expect("pair")
    d.close()


def test_a_failed_wait_releases_exactly_its_slot():
    d = Driver(make())
    assert d.submit("large", "host") == OK
    assert d.submit("small", "host") == OK
    rc, n, rec = d.wait(capacity=100)               # more candidates than the caller's capacity
    assert rc == CAPACITY and n == 100
    assert np.array_equal(rec, PC.batch_records("large")[:100])     # the first 100 of the order
    d.expect("small")                               # the other batch in flight: whole, and the next in line
    rc, n, buf = d.sync_batch("blank")              # nothing is in flight any more: a synchronous call is accepted
    want = PC.batch_records("blank")
    assert rc == OK and n == len(want) and np.array_equal(buf[: n * ST].reshape(n, ST), want)
    assert np.all(buf[n * ST:] == FILL)
    assert d.wait()[0] == STATE                     # a further wait: no batch in flight
    assert d.submit("pair", "device") == OK         # and the handle goes on
    d.expect("pair")
    d.close()


def test_nms_overflow_in_the_pipeline():
    """max_candidates 64 with the post-processing stage on: frame A holds more candidates than the stage's list, so there is
    no suppressed prefix to deliver (-4, *ncand = 0); the batch behind it is delivered, suppressed"""
    d = Driver(make(max_candidates=64, nms=0.5))
    fr = PC.frames()
    assert d.submit_host([fr["A"]]) == OK
    assert d.submit_host([fr["Z"]]) == OK
    rc, n, rec = d.wait(capacity=64)
    assert rc == CAPACITY and n == 0
    assert "max_candidates" in d.lib.pbd_last_error(d.h).decode()
    rc, n, rec = d.wait(capacity=64)
    want = PC.mirror(PC.records_of(("Z",)), 96, 128, 0.5)
    assert rc == OK and n == len(want) > 0
    assert np.array_equal(rec, want)
    assert d.wait(capacity=64)[0] == STATE
    d.close()


def test_refusals_in_flight_lose_nothing():
    d = Driver(make())
    w = d.hd.model_vector()                          # the handle's own vector, fetched while nothing is in flight
    fr = PC.frames()
    one = np.ascontiguousarray(fr["B"])
    assert d.submit("small", "host") == OK
    assert d.submit("large", "device") == OK
    # two batches in flight: PBD_ERR_STATE, whatever the call
    assert d.submit("blank", "host") == STATE
    assert d.submit("blank", "device") == STATE
    assert d.sync_batch("blank")[0] == STATE
    assert d.lib.pbd_set_nms(d.h, 1, C.c_float(0.5)) == STATE
    assert d.lib.pbd_set_model_vector(d.h, w.ctypes.data) == STATE
    d.expect("small")
    d.expect("large")                                # unsuppressed: the refused pbd_set_nms changed nothing
    # one batch in flight: refused by the argument checks, before the slot is touched
    assert d.submit("pair", "host") == OK
    four = [one] * (PC.MAX_BATCH + 1)
    assert d.submit_host(four) == INVALID            # nframes > max_batch
    assert d.submit_device(four) == INVALID
    assert d.lib.pbd_detect_batch_submit(d.h, 1, None, 64, 80, 3, 240) == INVALID                   # no frame array
    ptrs = (C.c_void_p * 2)(one.ctypes.data, None)
    assert d.lib.pbd_detect_batch_submit(d.h, 2, ptrs, 64, 80, 3, 240) == INVALID                   # a null frame in the array
    assert d.lib.pbd_detect_batch_device_submit(d.h, 1, None, 64, 80, 3) == INVALID                 # no device frames
    assert d.submit("blank", "host") == OK           # the free slot is still free
    assert d.submit("small", "host") == STATE        # and now both are taken
    d.expect("pair")
    d.expect("blank")
    assert d.wait()[0] == STATE
    d.close()


def _records(hd, cands):
    return hd.pack_candidates(cands).astype(np.int32).reshape(-1, ST)


def test_pool_failed_wait_moves_on_to_the_next_lane():
    """DetectorPool of three: the first wait fails with PBD_ERR_CAPACITY; its lane's slot is released, so the pool's cursor moves
    on: the other two batches come back, in order, and a second round of three is right."""
    import torch
    pool = detector.DetectorPool(PC.model(), n=3, device=0, max_batch=PC.MAX_BATCH, max_candidates=CAP)
    try:
        for name in ("large", "blank", "small"):
            pool.submit_batch(PC.batch_frames(name))
        assert pool.pending == 3 and pool.ready_before_next_submit
        with pytest.raises(PbdError) as e:
            pool.wait_batch(capacity=8, raw=True)
        assert e.value.code == CAPACITY
        assert pool.pending == 2
        got = _records(pool.dets[1].hd, pool.wait_batch(capacity=8))
        assert np.array_equal(got, PC.batch_records("blank"))
        got = _records(pool.dets[2].hd, pool.wait_batch())
        assert np.array_equal(got, PC.batch_records("small"))
        assert pool.pending == 0 and not pool.ready_before_next_submit
        dev = []
        for name in ("pair", "small", "large"):     # second round: lane 0 first again, device form
            fr = PC.batch_frames(name)
            dev.append(torch.from_numpy(np.stack(fr)).cuda())
            pool.submit_batch_device(dev[-1].data_ptr(), len(fr), fr[0].shape[0], fr[0].shape[1], fr[0].shape[2])
        for name in ("pair", "small", "large"):
            buf, n = pool.wait_batch(raw=True)
            assert np.array_equal(np.array(buf[: n * ST]).reshape(n, ST), PC.batch_records(name)), name
        assert pool.pending == 0
        with pytest.raises(PbdError) as e:
            pool.wait_batch()
        assert e.value.code == STATE and pool.pending == 0
    finally:
        pool.close()
