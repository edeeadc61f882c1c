"""The demo harness's --augment flag (host/demo.cpp): the image's augmented copy goes through PartsBasedDetector<T>::augmentFrames
(include/pbd_host.hpp -> pbd_augment_frames) and the file written holds the bytes of the numpy yardstick (augment.rotate_ref, fed
the coefficients pbd_augment_plan reports)."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import augment as A
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


def _write_pnm(path, im):
    with open(path, "wb") as fh:
        fh.write(b"P%d\n%d %d\n255\n" % (6 if im.shape[2] == 3 else 5, im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())


def _read_pnm(path):
    """a binary PPM / PGM as rows x cols x channels in BGR order"""
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    cols, rows = (int(v) for v in dims.split())
    cn = {b"P6": 3, b"P5": 1}[magic]
    assert maxval == b"255" and len(body) == rows * cols * cn
    return np.frombuffer(body, np.uint8).reshape(rows, cols, cn)[:, :, ::-1]


@pytest.mark.parametrize("arg,degrees,mirror,cn", [("15,mirror", 15.0, True, 3), ("-33.3", -33.3, False, 3), ("0,mirror", 0.0, True, 3),
                                                   ("90,mirror", 90.0, True, 1)])
def test_augment_writes_the_yardsticks_bytes(demo, tmp_path, arg, degrees, mirror, cn):
    mpath, ipath, opath = str(tmp_path / "model.yml"), str(tmp_path / "im.pnm"), str(tmp_path / "out.pnm")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    im = np.ascontiguousarray(synth.synthetic_frame(9, 61, 83, 3)[:, :, :cn])
    _write_pnm(ipath, im)
    r = subprocess.run([DEMO, mpath, ipath, "--augment", arg, opath], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows, cols, coef = A.plan_c(61, 83, degrees)
    want = A.rotate_ref(im, degrees, mirror, coef if degrees else None)
    assert r.stdout == "augment %d %d\n" % (rows, cols)
    got = _read_pnm(opath)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_augment_refuses_a_bad_argument(demo, tmp_path):
    mpath, ipath = str(tmp_path / "model.yml"), str(tmp_path / "im.ppm")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    _write_pnm(ipath, synth.synthetic_frame(9, 40, 56, 3))
    for arg in ("15,flip", "mirror", "15,mirrorx"):
        r = subprocess.run([DEMO, mpath, ipath, "--augment", arg, str(tmp_path / "o.ppm")], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--augment" in r.stderr, arg
