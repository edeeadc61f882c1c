"""host/pbd_demo --depth: the C++ host's PartsBasedDetector<T>::boundingBoxes3D (pbd_boxes3d) on a 16-bit PGM against the
Python mirror Candidate.boundingBox3D on the demo's own reported candidates; without --depth the output is unchanged."""
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, synth
from partsbaseddetector_amd.detector import Candidate
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--device-nms", "0.1"], ["--double", "--nms", "0.1", "--top", "3"]])
def test_demo_depth_matches_mirror(demo, tmp_path, flags):  # noqa: F811
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    depth = synth.synthetic_depth(21, 120, 90, np.uint16)           # another size than the colour frame
    dpath = tmp_path / "depth.pgm"
    dpath.write_bytes(b"P5\n90 120\n65535\n" + depth.astype(">u2").tobytes())
    plain = subprocess.run([demo, mpath, ipath] + flags, capture_output=True, text=True)
    r = subprocess.run([demo, mpath, ipath] + flags + ["--depth", str(dpath)], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert "box3d" not in plain.stdout
    lines = r.stdout.splitlines()
    assert [ln for ln in lines if not ln.startswith("box3d ")] == plain.stdout.splitlines()
    _, cands = _parse(r.stdout)
    boxes = [[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("box3d ")]
    assert 0 < len(cands) == len(boxes)
    for (_, _, parts), got in zip(cands, boxes):
        c = Candidate(parts=parts, confidence=np.zeros(len(parts), np.float32), component=0)
        want = c.boundingBox3D(im.shape, depth)
        np.testing.assert_array_equal(np.array(got), np.array(want))   # %.17g round-trips a double; NaN prints as nan
