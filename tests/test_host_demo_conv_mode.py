"""pbd_demo --conv-mode N: the C++ host's PartsBasedDetector<T> / FrameStream<T> conv_mode argument."""
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, synth
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--staged"], ["--stream", "2", "3"]])
def test_demo_fp64_matrix_mode_matches_oracle(demo, oracle, tmp_path, flags):  # noqa: F811
    model = M.synthetic_tiny_model(thresh=0.7)
    im = synth.synthetic_frame(5, 96, 128, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    r = subprocess.run([demo, mpath, ipath, "--double", "--conv-mode", "4"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if "--stream" in flags:
        assert "results identical" in r.stdout
    n, got = _parse(r.stdout)
    want = oracle.detect(model.flatten(), im, dtype=np.float64)
    assert n == len(want) == len(got) > 0
    want_map = {(w["level"], w["component"], w["root_y"], w["root_x"]): w for w in want}
    for key, score, parts in got:
        w = want_map[key]
        assert np.float32(w["score"]) == score and np.array_equal(parts, w["parts"])


def test_demo_fp64_matrix_mode_refuses_float(demo, tmp_path):  # noqa: F811
    """refused by pbd_create before it looks for a device: the same answer with or without a GPU"""
    model = M.synthetic_tiny_model()
    im = synth.synthetic_frame(5, 32, 40, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    r = subprocess.run([demo, mpath, ipath, "--conv-mode", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "PBD_CONV_MFMA_F64 needs PBD_REAL_F64" in r.stderr, r.stderr
