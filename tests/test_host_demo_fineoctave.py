"""host/pbd_demo --fine-octave (PartsBasedDetector<T>::setFineOctave, include/pbd_host.hpp): the usage text names the flag (no GPU
needed), and on the GPU the demo lists the records of the numpy rule (partsbaseddetector_amd/fineoctave.py)."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage as FS
from partsbaseddetector_amd import fineoctave as F
from partsbaseddetector_amd import model as M, synth

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
    assert r.returncode != 0 and "--fine-octave" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--double"], ["--stream", "2", "3"], ["--staged"], ["--pad", "1,3"]],
                         ids=["float", "double", "stream", "staged", "pad"])
def test_demo_prints_the_yardsticks_records(demo, tmp_path, flags):
    model = M.synthetic_tiny_model(thresh=0.6)
    im = synth.synthetic_frame(31, 60, 84, 3)
    mpath, ipath = str(tmp_path / "model.yml"), str(tmp_path / "frame.ppm")
    FS.serialize(model, mpath)
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())          # PPM stores RGB; the demo hands BGR to detect()
    dtype = np.float64 if "--double" in flags else np.float32
    pad = (1, 3) if "--pad" in flags else (0, 0)
    loaded = FS.deserialize(mpath)
    want = F.detect_ref(loaded, im, True, pad[0], pad[1], dtype)
    bare = F.detect_ref(loaded, im, False, pad[0], pad[1], dtype)
    assert len(want) > len(bare) >= 1 and any(r["level"] < 5 for r in want)
    r = subprocess.run([demo, mpath, ipath, "--fine-octave", "--top", "100000"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cand ")]
    assert f"Number of candidates: {len(want)}" in r.stdout and len(got) == len(want)
    key = sorted(((w["level"], w["component"], w["root_y"], w["root_x"]), w["parts"].ravel().tolist()) for w in want)
    assert sorted(((int(t[1]), int(t[2]), int(t[3]), int(t[4])), [int(v) for p in t[6:] for v in p.split(",")]) for t in got) == key
