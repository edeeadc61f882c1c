"""pbdhost::FrameStream<float> (include/pbd_host.hpp) on DIFFERENT frames: order of the results, and what a failed next() leaves
behind.  `pbd_demo --stream` sends one image N times, so a result handed back from the wrong handle passes its check; here
tests/host_stream_check.cpp streams distinct frames and prints every frame's list, which must be the CPU oracle's for that frame
(tests/pipeline_cases.py) after Candidate::sort's descending order.  std::sort leaves the order among equal scores open, so the
comparison is: printed scores never increase, and the printed records equal the oracle's once both are ordered by
(score descending, level, component, root_y, root_x)."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_cases as PC
from partsbaseddetector_amd import filestorage as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stream_check(tmp_path_factory):
    """the program, compiled once with host/Makefile's flags against include/ and the built library; model and frames written"""
    from partsbaseddetector_amd import build
    build.build_hip()
    d = tmp_path_factory.mktemp("host_stream")
    exe = str(d / "host_stream_check")
    libdir = os.path.join(ROOT, "partsbaseddetector_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "host_stream_check.cpp"), "-L" + libdir, "-lpbd_hip", "-lz",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    mpath = str(d / "model.yml")
    FS.serialize(PC.model(), mpath)
    paths = {}
    for name, im in PC.frames().items():
        paths[name] = str(d / f"{name}.ppm")
        with open(paths[name], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
            fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())      # PPM stores RGB; readPNM hands BGR to the stream
    return exe, mpath, paths


def run(stream_check, handles, capacity, names):
    exe, mpath, paths = stream_check
    r = subprocess.run([exe, mpath, str(handles), str(capacity)] + [paths[n] for n in names], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-600:], r.stderr[-2000:])
    reports, cur = [], None
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "frame":
            assert int(t[1]) == len(reports)
            cur = []
            reports.append(cur)
        elif t[0] == "error":
            cur.append(int(t[1]))
        else:
            assert t[0] == "cand"
            parts = [int(v) for p in t[6:] for v in p.split(",")]
            rec = np.zeros(PC.stride(), np.int32)
            rec[:8] = (0, int(t[2]), int(t[1]), int(t[4]), int(t[3]), 0, len(parts) // 4, 0)
            rec[5] = np.float32(t[5]).view(np.int32)                       # %.9g round-trips a float
            rec[8:8 + len(parts)] = parts
            cur.append(rec)
    assert len(reports) == len(names)
    return reports


def canonical(rec):
    """records ordered by (score descending, level, component, root_y, root_x)"""
    score = rec[:, 5].copy().view(np.float32)
    return rec[np.lexsort((rec[:, 3], rec[:, 4], rec[:, 1], rec[:, 2], -score.astype(np.float64)))]


def check_list(printed, name):
    want = PC.frame_records(name)
    assert all(isinstance(r, np.ndarray) for r in printed), (name, printed[:1])
    got = np.array(printed, np.int32).reshape(-1, PC.stride())
    assert got.shape == want.shape, (name, got.shape, want.shape)
    score = got[:, 5].copy().view(np.float32)
    assert np.all(score[:-1] >= score[1:]), name                           # Candidate::sort: descending
    assert np.array_equal(canonical(got), canonical(want)), name


def test_stream_returns_every_frame_its_own_list_in_submission_order(stream_check):
    names = ["A", "B", "Z", "C", "B", "A"]
    reports = run(stream_check, 3, 1 << 16, names)
    for printed, name in zip(reports, names):
        check_list(printed, name)


def test_stream_recovers_after_a_failed_next(stream_check):
    """capacity 8 (the handles' max_candidates): A and B hold more, the constant frames fewer.  A next() that throws
    PBD_ERR_CAPACITY has consumed its frame: the following frames' lists still come back, each from its own handle."""
    names = ["A", "Z", "B", "Z64"]
    reports = run(stream_check, 2, 8, names)
    for i in (0, 2):
        assert len(reports[i]) == 1 and isinstance(reports[i][0], int) and reports[i][0] == -4, (i, reports[i][:1])
    check_list(reports[1], "Z")
    check_list(reports[3], "Z64")
