"""detector.DetectorPool's bookkeeping over stand-in lanes (no GPU, no handle): which lane every submit and wait goes to, and what
a failed wait leaves behind.

pbd_detect_batch_wait releases its slot before it can fail (include/pbd.h), so a lane whose wait_batch raised holds nothing any
more: the pool's cursor has to move on with every outcome of the lane call, or every later wait_batch() returns to that lane and
gets PBD_ERR_STATE while the other lanes' results become unreachable."""
import pytest

from partsbaseddetector_amd.detector import DetectorPool, PbdError


class Lane:
    """records its calls; holds at most one batch, like a pool lane; raises on request after releasing what it held"""

    def __init__(self, name, log):
        self.name, self.log, self.held, self.fail_next_wait, self.refuse_next_submit = name, log, [], False, False

    def submit_batch(self, frames, depths=None):
        self.log.append(("submit", self.name, frames))
        if self.refuse_next_submit:
            self.refuse_next_submit = False
            raise PbdError(-1, "refused by the argument check")
        self.held.append(frames)

    def submit_batch_device(self, ptr, nframes, rows, cols, cn):
        self.submit_batch(ptr)

    def wait_batch(self, capacity=None, raw=False):
        self.log.append(("wait", self.name, capacity, raw))
        if not self.held:
            raise PbdError(-5, "no batch in flight")               # what a handle answers once its slot is released
        tag = self.held.pop(0)                                      # released whatever happens below
        if self.fail_next_wait:
            self.fail_next_wait = False
            raise PbdError(-4, f"{tag}: more candidates than the capacity")
        return ("result", tag)


def make_pool(n=3):
    log = []
    pool = DetectorPool.__new__(DetectorPool)                      # without __init__'s handles
    pool.dets = [Lane(i, log) for i in range(n)]
    pool._submitted = pool._collected = 0
    return pool, log


def state(pool):
    return pool.pending, pool.ready_before_next_submit


def test_round_robin_order_without_failures():
    pool, log = make_pool(3)
    assert state(pool) == (0, False)
    for i, tag in enumerate("abc"):
        pool.submit_batch(tag)
        assert state(pool) == (i + 1, i == 2)
    assert pool.wait_batch(capacity=7, raw=True) == ("result", "a")
    assert state(pool) == (2, False)
    pool.submit_batch_device("d", 1, 2, 3, 4)                      # lane 0 again: it is the one that was collected
    assert state(pool) == (3, True)
    assert [pool.wait_batch() for _ in range(3)] == [("result", t) for t in "bcd"]
    assert state(pool) == (0, False)
    assert [(e[0], e[1]) for e in log] == [("submit", 0), ("submit", 1), ("submit", 2), ("wait", 0), ("submit", 0),
                                           ("wait", 1), ("wait", 2), ("wait", 0)]
    assert log[3] == ("wait", 0, 7, True)                          # capacity and raw reach the lane


@pytest.mark.parametrize("failing", [0, 1, 2])
def test_a_failed_wait_at_each_position_of_a_round_moves_on(failing):
    pool, log = make_pool(3)
    for tag in "abc":
        pool.submit_batch(tag)
    pool.dets[failing].fail_next_wait = True
    got = []
    for i in range(3):
        assert state(pool) == (3 - i, i == 0)
        if i == failing:
            with pytest.raises(PbdError) as e:
                pool.wait_batch()
            assert e.value.code == -4                               # the lane's own error reaches the caller
            got.append(None)
        else:
            got.append(pool.wait_batch())
        assert state(pool) == (2 - i, False)                        # one batch fewer, failed or not
    assert got == [None if i == failing else ("result", t) for i, t in enumerate("abc")]
    assert [e[:2] for e in log[3:]] == [("wait", 0), ("wait", 1), ("wait", 2)]      # every lane exactly once, in order
    # the second round starts on lane 0 again and is complete
    for tag in "def":
        pool.submit_batch(tag)
    assert state(pool) == (3, True)
    assert [pool.wait_batch() for _ in range(3)] == [("result", t) for t in "def"]
    assert [e[:2] for e in log[6:]] == [("submit", 0), ("submit", 1), ("submit", 2), ("wait", 0), ("wait", 1), ("wait", 2)]
    assert state(pool) == (0, False)


def test_a_failed_wait_with_a_partly_filled_pool():
    pool, log = make_pool(3)
    pool.submit_batch("a")
    pool.submit_batch("b")
    pool.dets[0].fail_next_wait = True
    with pytest.raises(PbdError):
        pool.wait_batch()
    assert state(pool) == (1, False)
    pool.submit_batch("c")                                          # lane 2: the submit cursor is not touched by the failure
    pool.submit_batch("d")                                          # lane 0: free again after its failed wait
    assert state(pool) == (3, True)
    assert [pool.wait_batch() for _ in range(3)] == [("result", t) for t in "bcd"]
    assert [e[:2] for e in log] == [("submit", 0), ("submit", 1), ("wait", 0), ("submit", 2), ("submit", 0), ("wait", 1),
                                    ("wait", 2), ("wait", 0)]


def test_refusals_change_neither_counter():
    pool, log = make_pool(2)
    with pytest.raises(PbdError) as e:
        pool.wait_batch()                                           # nothing submitted: the pool's own refusal
    assert e.value.code == -5 and state(pool) == (0, False) and log == []
    pool.submit_batch("a")
    pool.dets[1].refuse_next_submit = True
    with pytest.raises(PbdError) as e:
        pool.submit_batch("x")                                      # refused by the lane: nothing was enqueued
    assert e.value.code == -1 and state(pool) == (1, False)
    pool.submit_batch("b")                                          # the same lane takes the next batch
    assert state(pool) == (2, True)
    for form in (lambda: pool.submit_batch("y"), lambda: pool.submit_batch_device("y", 1, 2, 3, 4)):
        with pytest.raises(PbdError) as e:
            form()                                                  # every lane holds a batch: refused by the pool
        assert e.value.code == -5 and state(pool) == (2, True)
    assert [e[:2] for e in log] == [("submit", 0), ("submit", 1), ("submit", 1)]   # the pool's refusals reached no lane
    assert [pool.wait_batch(), pool.wait_batch()] == [("result", "a"), ("result", "b")]
    with pytest.raises(PbdError):
        pool.wait_batch()
    assert state(pool) == (0, False)
    assert [e[:2] for e in log[3:]] == [("wait", 0), ("wait", 1)]   # the last refusal reached no lane either
