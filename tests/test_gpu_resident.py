"""The resident result of one long-lived handle under every order of writer and reader calls (resident_cases.py): after any two
writers every reader gives the bytes of the last effective writer's scene or the status code the table's cell names, twice over;
options changed between a write and a read re-emit the resident list as their numpy mirrors say; seeded walks mix writers, readers
and options on one handle; a handle with fp16-resident responses gives what a fresh handle gives after the last writer alone; and
while a batch is in flight every reader is refused.  Every comparison is of bytes or of integers; nothing has a tolerance."""
import pytest

import resident_cases as RC
from partsbaseddetector_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = tuple(w.name for w in RC.WRITERS)
FRAME_OFFSET = 3


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


class Lived:
    """one handle per key that lives across the cases of a test and the state the table says it is in; a case that fails leaves
    a handle nobody can vouch for, so the next case starts a new one"""

    def __init__(self):
        self.held = {}

    def get(self, key, dtype, conv_mode=_lib.CONV_EXACT):
        if key not in self.held:
            self.held[key] = (RC.new_handle(dtype, conv_mode), RC.State())
        return self.held[key]

    def drop(self, key):
        hd, _ = self.held.pop(key, (None, None))
        if hd is not None:
            hd.close()

    def close(self):
        for key in list(self.held):
            self.drop(key)


@pytest.fixture(scope="module")
def lived():
    keeper = Lived()
    yield keeper
    keeper.close()


def short(v):
    if isinstance(v, tuple):
        return tuple(f"<{len(x)} bytes #{hash(x) & 0xffff:04x}>" if isinstance(x, bytes) else x for x in v)
    return v


def differences(got, want):
    if [k for k, _ in got] != [k for k, _ in want]:
        return [("addresses", [k for k, _ in got][:6], [k for k, _ in want][:6])]
    return [(k, short(g), short(w)) for (k, g), (_, w) in zip(got, want) if g != w]


def check_reader(hd, state, reader, dtype, st, context):
    """the reader twice (a reader does not change the result): the problems found, each with the table's cell"""
    want = RC.want(state, reader, dtype, st, FRAME_OFFSET)
    cell = state.cell(reader)
    problems = []
    for again in (False, True):
        bad = differences(RC.read(hd, state, reader, dtype, st, FRAME_OFFSET), want)
        if bad:
            problems.append((context, reader, "again" if again else "first", f"{cell.kind}: {cell.quote}", len(bad), bad[:3]))
    if reader == "max_marginals" and state.kind(reader) == RC.VALUE:
        state.wrote(RC.WRITER["max_marginals"], RC.arg_scene(state, dtype).nframes - 1)
    return problems


def check_readers(hd, state, dtype, context, st=None, readers=RC.READERS):
    """every reader; the state follows the table whatever a reader gave, so one case shows every cell that is wrong"""
    return [p for reader in readers for p in check_reader(hd, state, reader, dtype, st, context)]


def report(problems):
    assert not problems, (len(problems), problems[:8])


def check_plain_detect(hd, state, dtype, context):
    """nothing a sequence did leaks into the detect path"""
    RC.run_writer(hd, state, "detect", dtype)
    assert state.stack == ["detect"], context


# ---- a) every ordered pair of writers, then every reader -------------------------------------------------------------------------
@pytest.mark.parametrize("first", NAMES)
@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_pairwise(lived, dtype, first):
    hd, state = lived.get(dtype, dtype)
    try:
        problems = []
        for second in NAMES:
            RC.run_writer(hd, state, first, dtype)
            RC.run_writer(hd, state, second, dtype)
            problems += check_readers(hd, state, dtype, (first, second, tuple(state.stack)))
        check_plain_detect(hd, state, dtype, first)
        report(problems)
    except BaseException:
        lived.drop(dtype)
        raise


# ---- b) options changed between the write and the read ----------------------------------------------------------------------------
DEPTH = (525.0, 450.0, 0.35)
OPTIONS = (RC.settings(walk="argmax"), RC.settings(nms=0.3), RC.settings(root_nms=2), RC.settings(top_k=7), RC.settings(dprune=DEPTH),
           RC.settings(walk="argmax", nms=0.3, root_nms=2, top_k=7, dprune=DEPTH), RC.settings(root_nms=1, top_k=40))


def apply(hd, st):
    hd.set_walk(_lib.WALK_ARGMAX if st["walk"] == "argmax" else _lib.WALK_REFERENCE)
    hd.set_nms(st["nms"])
    hd.set_root_nms(st["root_nms"])
    hd.set_top_k(st["top_k"])
    if st["dprune"] is None:
        hd.set_depth_prune(None)
    else:
        hd.set_depth_prune(*st["dprune"])


@pytest.mark.parametrize("writer", ["detect", "detect_batch", "detect_frames"])
@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_options_between_write_and_read(dtype, writer):
    hd, state = RC.new_handle(dtype), RC.State()
    try:
        RC.run_writer(hd, state, writer, dtype)
        sc = RC.arg_scene(state, dtype)
        for st in OPTIONS + (RC.OFF,):
            apply(hd, st)
            for reader in ("argmin_device_out", "dp_argmin", "argmin_device_out"):
                if reader == "argmin_device_out" and st["dprune"] is not None:
                    hd.bind_depth(list(RC.depth_images(sc.name)))           # the next call consumes the binding
                want = RC.want(state, reader, dtype, st, FRAME_OFFSET)
                bad = differences(RC.read(hd, state, reader, dtype, st, FRAME_OFFSET), want)
                assert not bad, (writer, st, reader, bad[:2])
        full = RC.want(state, "argmin_device_out", dtype, RC.OFF, FRAME_OFFSET)[0][1]
        assert full[1] == len(sc.records()) and all(
            RC.want(state, "argmin_device_out", dtype, st, FRAME_OFFSET)[0][1][1] < full[1] for st in OPTIONS[1:])
        report(check_readers(hd, state, dtype, (writer, "options off again")))      # the planes never changed
        check_plain_detect(hd, state, dtype, writer)
    finally:
        hd.close()


# ---- c) seeded walks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,dtype", list(zip(RC.WALK_SEEDS, ("float32", "float64", "float32"))))
def test_seeded_walk(seed, dtype):
    hd, state, st = RC.new_handle(dtype), RC.State(), dict(RC.OFF)
    steps = RC.walk_steps(seed)
    done = []
    try:
        for step in steps:
            done.append(step)
            if step[0] == "write":
                RC.run_writer(hd, state, step[1], dtype, st)
            elif step[0] == "read":
                report(check_reader(hd, state, step[1], dtype, st, len(done)))
            else:
                key = step[1][len("set_"):]
                st[key] = step[2]
                apply(hd, st)
        report(check_readers(hd, state, dtype, "end of the walk", st))
        apply(hd, RC.OFF)
        check_plain_detect(hd, state, dtype, seed)
    except BaseException:
        print(f"\nwalk {seed} ({dtype}) failed at step {len(done)}; the steps so far:")
        for i, s in enumerate(done):
            print(f"  {i + 1:2d} {s}")
        raise
    finally:
        hd.close()


# ---- d) fp16-resident responses: history does not matter ------------------------------------------------------------------------------
HALF_WRITERS = ("detect", "detect_a2", "detect_s", "detect_g", "detect_batch", "detect_batch_device_out", "submit_wait",
                "detect_frames", "detect_frames_device_out", "detect_latent")
HALF_READERS = RC.STAGE_READERS + ("examples", "part_scores", "argmin_device_out")
_alone = {}


def alone(name):
    """what a fresh PBD_CONV_MFMA_F16_ANY handle returns for writer `name` and gives every reader afterwards"""
    if name not in _alone:
        hd, state = RC.new_handle("float32", _lib.CONV_MFMA_F16_ANY), RC.State()
        try:
            returned = RC.run_writer(hd, state, name, "float32", check=False)
            reads = {r: RC.read(hd, state, r, "float32", None, FRAME_OFFSET) for r in HALF_READERS}
            _alone[name] = ([a.tobytes() for a in returned], reads)
        finally:
            hd.close()
    return _alone[name]


@pytest.mark.parametrize("first", HALF_WRITERS)
def test_fp16_resident_pairwise(lived, first):
    """no bit-exact oracle exists for this mode (its accuracy is pinned in test_gpu_conv_mfma_any.py): the expected bytes are a
    fresh handle's after the last writer alone.  A status cell is the table's, as in the exact mode."""
    key = "half"
    hd, state = lived.get(key, "float32", _lib.CONV_MFMA_F16_ANY)
    try:
        for second in HALF_WRITERS:
            RC.run_writer(hd, state, first, "float32", check=False)
            returned = RC.run_writer(hd, state, second, "float32", check=False)
            want_returned, want_reads = alone(second)
            assert [a.tobytes() for a in returned] == want_returned, (first, second, "returned")
            for reader in HALF_READERS:
                table = RC.want(state, reader, "float32", None, FRAME_OFFSET)
                for again in (False, True):
                    got = RC.read(hd, state, reader, "float32", None, FRAME_OFFSET)
                    bad = differences(got, want_reads[reader])
                    assert not bad, (first, second, reader, again, bad[:4])
                    # where the table names a status code the handle gives it; where it names bytes, bytes came
                    codes = [(k, g) for (k, g), (_, w) in zip(got, table)
                             if isinstance(w, int) != isinstance(g, int) or (isinstance(w, int) and g != w)]
                    assert not codes, (first, second, reader, codes[:4])
            assert RC.code_of(lambda: hd.max_marginals(0))[0] == RC.UNSUPPORTED      # the mode is looked at before the result
            assert RC.code_of(lambda: hd.get_marginals(0, _lib.MM_VALUES, 4, 4))[0] == RC.STATE
        plain = RC.run_writer(hd, state, "detect", "float32", check=False)
        assert [a.tobytes() for a in plain] == alone("detect")[0], first
        # the mode is the one meant: its responses are not the exact mode's
        resp = dict(RC.read(hd, state, "stage_responses", "float32"))[("responses", 0, 0)][1]
        assert resp != RC.scene("a", "float32").plane_bytes("responses", 0, 0)
    except BaseException:
        lived.drop(key)
        raise


# ---- e) pipelined ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_readers_are_refused_in_flight_and_see_the_last_batch_after(dtype):
    hd, state = RC.new_handle(dtype), RC.State()
    try:
        RC.run_writer(hd, state, "detect_s", dtype)                           # an older, smaller result to fall back on by mistake
        b3, a2 = RC.scene("b3", dtype), RC.scene("a2", dtype)
        hd.submit_batch(list(b3.frames))
        hd.submit_batch(list(a2.frames))
        refused = RC.State()                                                  # sizes the buffers for refusals only
        for nwaited in (0, 1):
            for reader in RC.READERS:
                got = RC.read(hd, refused, reader, dtype, None, FRAME_OFFSET)
                assert got and all(v == RC.STATE for _, v in got), \
                    (RC.Q_FLIGHT, nwaited, reader, [(k, short(v)) for k, v in got if v != RC.STATE][:4])
            for name in ("conv_set_filters", "set_model_vector", "set_thresh", "warp_positives", "set_level_shard", "grid_nms",
                         "detect", "detect_frames", "detect_latent", "features_pyramid"):
                assert RC.code_of(lambda: RC.run_writer(hd, RC.State(), name, dtype))[0] == RC.STATE, (nwaited, name)
            got = RC._list(hd, hd.lib.pbd_detect_batch_wait)
            RC._same(got, RC.emitted((b3, a2)[nwaited], RC.OFF), ("wait", nwaited))
        state.wrote(RC.WRITER["submit_wait"])
        assert RC.Q_PIPE in state.cell("stage_rootv").quote
        report(check_readers(hd, state, dtype, "after the second wait"))
        check_plain_detect(hd, state, dtype, "pipelined")
    finally:
        hd.close()
