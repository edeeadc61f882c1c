"""host/pbd_demo --device-nms: the C++ host's PartsBasedDetector<T>::setNonMaximaSuppression (pbd_set_nms) against the Python
mirror of the callers' post-step on the same detections: same candidates, same order."""
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, synth
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--double"], ["--stream", "2", "3"]])
def test_demo_device_nms_matches_python_mirror(demo, tmp_path, flags):  # noqa: F811
    import torch
    torch.cuda.init()
    from partsbaseddetector_amd import detector as D
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    r = subprocess.run([demo, mpath, ipath, "--device-nms", "0.1"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "After device NMS" in r.stdout
    _, got = _parse(r.stdout)
    det = D.PartsBasedDetector(device=0, dtype=np.float64 if "--double" in flags else np.float32)
    det.distributeModel(model)
    cands = det.detect(im)
    D.Candidate.sort(cands)
    D.Candidate.nonMaximaSuppression(im.shape, cands, float(np.float32(0.1)))
    assert 0 < len(got) == len(cands)
    assert [k for k, _, _ in got] == [(c.level, c.component, c.root[1], c.root[0]) for c in cands]
    for (_, score, parts), c in zip(got, cands):
        assert score == np.float32(c.score()) and np.array_equal(parts, c.parts)
    det.hd.close()
