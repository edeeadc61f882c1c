"""The demo harness's --also flag (host/demo.cpp): the first image and every --also image go through ONE
PartsBasedDetector<T>::detectBatch call (include/pbd_host.hpp -> pbd_bind.hpp detect_batch -> pbd_detect_frames), and each
image's candidates print exactly as a single run of that image prints them."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage as FS
from partsbaseddetector_amd import model as M, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "host", "pbd_demo")


@pytest.fixture(scope="module")
def demo():
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return DEMO


def _write_ppm(path, im):
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())


def _run(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("flags", [[], ["--double"], ["--device-nms", "0.1"], ["--double", "--device-nms", "0.3"],
                                   ["--nms", "0.2", "--top", "5"]])
def test_also_prints_what_single_runs_print(demo, tmp_path, flags):
    mpath = str(tmp_path / "model.yml")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    paths = []
    for i, (r, c) in enumerate([(96, 128), (120, 150), (81, 103)]):
        p = str(tmp_path / f"im{i}.ppm")
        _write_ppm(p, synth.synthetic_frame(50 + i, r, c, 3))
        paths.append(p)
    singles = [_run([mpath, p] + flags) for p in paths]
    assert all("Number of candidates: " in s for s in singles)
    assert sum(s.count("\ncand ") + s.startswith("cand ") for s in singles) > 0
    batch = _run([mpath, paths[0], "--also", paths[1], "--also", paths[2]] + flags)
    assert batch == "".join(singles)


def test_also_refuses_staged(demo, tmp_path):
    mpath = str(tmp_path / "model.yml")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    p = str(tmp_path / "im.ppm")
    _write_ppm(p, synth.synthetic_frame(7, 96, 128, 3))
    r = subprocess.run([DEMO, mpath, p, "--also", p, "--staged"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--also" in r.stderr
