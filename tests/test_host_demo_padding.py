"""host/pbd_demo --pad X[,Y] (PartsBasedDetector<T>::setPadding, include/pbd_host.hpp): the usage text names the flag and a bad
value is refused (no GPU needed), and on the GPU the demo lists the candidates Python's setPadding gives."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage as FS
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
    assert r.returncode != 0 and "--pad" in r.stderr


@pytest.mark.parametrize("value", ["32", "2,40", "-1", "x", "2,3,4"])
def test_a_bad_value_is_refused(demo, value):
    r = subprocess.run([demo, "model.yml", "frame.ppm", "--pad", value], capture_output=True, text=True)
    assert r.returncode != 0 and "--pad takes" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("pad,flags", [("2", []), ("1,3", []), ("1,3", ["--double"]), ("2", ["--stream", "2", "3"]), ("2", ["--staged"])],
                         ids=["2", "1,3", "1,3-double", "2-stream", "2-staged"])
def test_demo_lists_what_python_finds(demo, tmp_path, pad, flags):
    from partsbaseddetector_amd import detector
    model = M.synthetic_tiny_model(thresh=0.6)
    im = synth.synthetic_frame(31, 120, 150, 3)
    mpath, ipath = str(tmp_path / "model.yml"), str(tmp_path / "frame.ppm")
    FS.serialize(model, mpath)
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())          # PPM stores RGB; the demo hands BGR to detect()
    px, py = (int(v) for v in (pad.split(",") * 2)[:2])
    det = detector.PartsBasedDetector(device=0, dtype=np.float64 if "--double" in flags else np.float32)
    det.distributeModel(FS.deserialize(mpath))
    try:
        bare = det.detect(im)
        det.setPadding(px, py)
        want = det.detect(im)
    finally:
        det.hd.close()
    assert len(want) > len(bare) >= 1
    assert any(np.any(c.parts[:, :2] < -4) for c in want)                  # parts outside the image were among them
    r = subprocess.run([demo, mpath, ipath, "--pad", pad, "--top", "100000"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cand ")]
    assert f"Number of candidates: {len(want)}" in r.stdout and len(got) == len(want)
    key = sorted(((c.level, c.component, c.root[1], c.root[0]), c.parts.ravel().tolist()) for c in want)
    assert sorted(((int(t[1]), int(t[2]), int(t[3]), int(t[4])), [int(v) for p in t[6:] for v in p.split(",")]) for t in got) == key
