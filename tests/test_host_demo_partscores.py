"""host/pbd_demo --part-scores (PartsBasedDetector<T>::partScores, include/pbd_host.hpp): the usage text names the flag and the
runs it cannot serve are refused (no GPU needed), and on the GPU the demo prints, per listed candidate and part, the cell, the
mixture and the bits of the four values of the numpy rule (partsbaseddetector_amd/partscores.py) on the oracle's maps."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import filestorage as FS
from partsbaseddetector_amd import model as M, synth
from partsbaseddetector_amd import partscores as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "host", "pbd_demo")


@pytest.fixture(scope="module")
def demo():
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return DEMO


def test_usage_names_the_flag(demo):
    r = subprocess.run([demo], capture_output=True, text=True)
    assert r.returncode != 0 and "--part-scores" in r.stderr


@pytest.mark.parametrize("args", [["--staged"], ["--stream", "2", "3"], ["--also", "other.ppm"]], ids=["staged", "stream", "also"])
def test_runs_without_one_resident_result_are_refused_before_anything_is_read(demo, args):
    r = subprocess.run([demo, "no_model.yml", "no_image.ppm", "--part-scores"] + args, capture_output=True, text=True)
    assert r.returncode != 0 and "--part-scores" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--double"], ["--walk", "argmax"], ["--double", "--walk", "argmax"]],
                         ids=["float", "double", "float_argmax", "double_argmax"])
def test_demo_prints_the_rules_bits(demo, tmp_path, flags):
    dtype = np.float64 if "--double" in flags else np.float32
    walk = "argmax" if "argmax" in flags else "reference"
    mpath, ipath = str(tmp_path / "model.yml"), str(tmp_path / "frame.ppm")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    flat = FS.deserialize(mpath).flatten()
    im = synth.synthetic_frame(31, 120, 150, 3)
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())          # PPM stores RGB; the demo hands BGR to detect()
    r = subprocess.run([demo, mpath, ipath, "--part-scores", "--top", "12"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cands = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cand ")]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("part_score ")]
    assert len(cands) == 12 and len(lines) == 12 * 3
    fm = E.FrameMaps(flat, im, dtype, walk=walk)
    for i, t in enumerate(cands):
        lvl, c, y, x = (int(v) for v in t[1:5])
        pl = fm.placement(lvl, c, x, y)
        want = PS.part_scores(flat, fm.resp(lvl), c, pl, dtype)
        for p in range(3):
            ln = lines[3 * i + p]
            assert [int(v) for v in ln[1:6]] == [i, p] + list(pl[p])
            got = np.array([float.fromhex(v) for v in ln[6:10]], dtype)
            assert got.tobytes() == want[p].tobytes(), (i, p)
        if walk == "argmax":                                              # the root's message is the score on the cand line
            assert np.float32(float.fromhex(lines[3 * i][7])) == np.float32(float(t[5]))
