"""host/pbd_demo --depth MAP --depth-prune FX,WIDTH,TOL (PartsBasedDetector<T>::setDepthPrune and detect(im, depth, .),
FrameStream<T>::submit(im, depth); include/pbd_host.hpp): the usage text names the flag and the argument refusals need no GPU; on
the GPU the demo lists the candidates Python's setDepthPrune gives."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage as FS
from partsbaseddetector_amd import model as M, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "host", "pbd_demo")
FX, WIDTH, TOL = 500.0, 40.0, 0.02


@pytest.fixture(scope="module")
def demo():
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return DEMO


def test_usage_names_the_flag(demo):
    r = subprocess.run([demo], capture_output=True, text=True)
    assert r.returncode != 0 and "--depth-prune fx,width,tol" in r.stderr


@pytest.mark.parametrize("args, word", [(["--depth-prune", "500,40"], "takes fx,width,tol"),
                                        (["--depth-prune", "500,40,0.1,7"], "takes fx,width,tol"),
                                        (["--depth-prune", "a,b,c"], "takes fx,width,tol"),
                                        (["--depth-prune", "500,40,0.1"], "needs --depth"),
                                        (["--depth", "d.pgm", "--staged", "--depth-prune", "500,40,0.1"], "not with --staged")])
def test_argument_refusals(demo, args, word):
    r = subprocess.run([demo, "model.yml", "frame.ppm"] + args, capture_output=True, text=True)   # refused before a file is opened
    assert r.returncode != 0 and word in r.stderr and "candidates" not in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--double"], ["--stream", "2", "3"]], ids=["float", "double", "stream"])
def test_demo_lists_what_python_keeps(demo, tmp_path, flags):
    from partsbaseddetector_amd import detector
    model = M.synthetic_tiny_model(thresh=-0.5)
    im = synth.synthetic_frame(61, 80, 96, 3)
    mpath, ipath, dpath = str(tmp_path / "model.yml"), str(tmp_path / "frame.ppm"), str(tmp_path / "depth.pgm")
    FS.serialize(model, mpath)
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())          # PPM stores RGB; the demo hands BGR to detect()
    det = detector.PartsBasedDetector(device=0, dtype=np.float64 if "--double" in flags else np.float32)
    det.distributeModel(FS.deserialize(mpath))
    try:
        full = det.detect(im)
        # blocks of 5 x 5 pixels hold, at random, the depth one of the levels' root widths expects, or a hole
        widths = sorted({int(c.parts[0][2]) for c in full})
        vals = np.rint(np.array([FX * WIDTH / w for w in widths] + [0.0]))
        idx = np.random.default_rng(5).integers(0, len(vals), (16, 20))
        depth = vals[np.kron(idx, np.ones((5, 5), np.int64))[:80, :96]].astype(np.uint16)
        det.setDepthPrune(FX, WIDTH, TOL)
        want = det.detect(im, depth)
    finally:
        det.hd.close()
    assert len(full) >= 1000 and len(full) // 4 <= len(want) <= 3 * len(full) // 4
    with open(dpath, "wb") as fh:                                          # a 16-bit PGM stores big-endian samples
        fh.write(b"P5\n96 80\n65535\n")
        fh.write(depth.astype(">u2").tobytes())
    r = subprocess.run([demo, mpath, ipath, "--depth", dpath, "--depth-prune", f"{FX},{WIDTH},{TOL}", "--top", "100000"] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert f"Number of candidates: {len(want)}" in r.stdout
    got = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("cand ")]
    key = sorted(((c.level, c.component, c.root[1], c.root[0]), c.parts.ravel().tolist()) for c in want)
    assert sorted(((int(t[1]), int(t[2]), int(t[3]), int(t[4])), [int(v) for p in t[6:] for v in p.split(",")]) for t in got) == key
