"""pbd_demo --conv-mode 5: the C++ host in PBD_CONV_MFMA_ANY on a mixed-size model file, against the Python detector in the
same mode; and the refusal of the mode for --double."""
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, synth
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)


@pytest.mark.gpu
def test_demo_any_mode_prints_the_python_detectors_candidates(demo, tmp_path):  # noqa: F811
    from partsbaseddetector_amd import _lib, detector
    model = M.synthetic_model(seed=31, pa=[0, 1, 1, 2], nmix=2, ksize=[3, 4, 7], thresh=0.7, name="mixed_demo")
    im = synth.synthetic_frame(5, 96, 128, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    r = subprocess.run([demo, mpath, ipath, "--conv-mode", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n, got = _parse(r.stdout)
    det = detector.PartsBasedDetector(device=0, conv_mode=_lib.CONV_MFMA_ANY)
    det.distributeModel(model)
    try:
        want = det.detect(im)
    finally:
        det.hd.close()
    assert n == len(want) == len(got) > 0
    want_map = {(c.level, c.component, c.root[1], c.root[0]): c for c in want}
    for key, score, parts in got:
        c = want_map[key]
        assert np.float32(c.score()) == score and np.array_equal(parts, c.parts)


def test_demo_any_mode_refuses_double(demo, tmp_path):  # noqa: F811
    """refused by pbd_create before it looks for a device: the same answer with or without a GPU"""
    model = M.synthetic_tiny_model()
    im = synth.synthetic_frame(5, 32, 40, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    for mode in ("5", "6"):
        r = subprocess.run([demo, mpath, ipath, "--double", "--conv-mode", mode], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "need PBD_REAL_F32" in r.stderr and "PBD_CONV_MFMA_F64" in r.stderr, r.stderr
