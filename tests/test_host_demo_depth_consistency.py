"""host/pbd_demo --depth-consistency: the C++ host's PartsBasedDetector<T>::filterCandidatesByDepth and detect(im, depth) with
setDepthConsistency on (pbd_depth_consistency, then pbd_suppress) against the numpy mirror; and the new pbd_bind.hpp /
pbd_host.hpp lines compile without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import consistency, detector
from partsbaseddetector_amd import model as M, synth
from test_host_demo import ROOT, _parse, _write_inputs, demo  # noqa: F401  (fixture)


def test_demo_usage_names_the_flag(demo):  # noqa: F811
    r = subprocess.run([demo], capture_output=True, text=True)
    assert "--depth-consistency" in r.stderr


def test_demo_refuses_the_flag_without_depth(demo, tmp_path):  # noqa: F811
    mpath, ipath = _write_inputs(tmp_path, M.synthetic_tiny_model(thresh=0.7), synth.synthetic_frame(1, 96, 80, 3))
    r = subprocess.run([demo, mpath, ipath, "--depth-consistency", "0.03"], capture_output=True, text=True)
    assert r.returncode != 0 and "--depth-consistency needs --depth" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--device-nms", "0.1"], ["--double", "--device-nms", "0.3"]])
def test_demo_depth_consistency_matches_mirror(demo, tmp_path, flags):  # noqa: F811
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    depth = np.full((160, 120), 2000, np.uint16)         # two flat surfaces: a record on one keeps, one across both drops
    depth[:, 60:] = 900
    dpath = tmp_path / "depth.pgm"
    dpath.write_bytes(b"P5\n120 160\n65535\n" + depth.astype(">u2").tobytes())
    z = "0.03"
    r = subprocess.run([demo, mpath, ipath] + flags + ["--top", "1000", "--depth", str(dpath), "--depth-consistency", z],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("depth_consistency ")][0]
    kept, dropped = int(line.split()[4]), int(line.split()[6])
    dtype = np.float64 if "--double" in flags else np.float32
    hd = detector.Handle(model, device=0, real_type=1 if dtype == np.float64 else 0)
    try:
        raw = detector.PartsBasedDetector(dtype=dtype)
        raw.distributeModel(model)
        rec = raw.hd.pack_candidates(raw.detect(im))
        want = consistency.filter_records(hd.flat, rec, [depth], float(np.float32(z)), dtype)
        assert (kept, dropped) == (len(want), len(rec) - len(want))
        assert 0 < kept < len(rec)
        overlap = float(flags[-1])
        sup = hd.suppress([(160, 120)], overlap, want)
        _, cands = _parse(r.stdout)
        assert len(cands) == len(sup)
        for (_, score, parts), w in zip(cands, sup):
            assert np.array_equal(parts, w[8:8 + 4 * len(parts)].reshape(-1, 4))
        raw.hd.close()
    finally:
        hd.close()


def test_bind_and_host_lines_compile(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
void use(pbdhost::PartsBasedDetector<float> &d, pbdhost::PartsBasedDetector<double> &e, const pbdhost::Image &im, const pbdhost::Image &depth,
         std::vector<pbdhost::Candidate> &c)
{
    d.setDepthConsistency(true, 0.03f);
    d.detect(im, depth, c);
    d.filterCandidatesByDepth(depth, c, 0.03f);
    d.suppress(im, c, 0.1f);
    e.setDepthConsistency(false);
    e.filterCandidatesByDepth(depth, c);
    e.suppress(im, c, 0.5f);
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
