"""A model loaded from a Matlab .mat file detects exactly as the same model loaded from FileStorage XML, and as the CPU
oracle, for T = float and T = double: the committed fixtures (tests/golden/make_matlab_fixtures.py) and a person-sized
model (26 parts x 6 mixtures) written at test time by matlab_model.serialize."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage, load_model_file, matlab_model, synth
from partsbaseddetector_amd import model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
XML = os.path.join(GOLDEN, "matlab_fixture.xml")
FRAMES = [(1, 96, 128, 3), (2, 120, 100, 1), (3, 160, 200, 3)]


def _key(c):
    return (c.level, c.component, c.root[1], c.root[0], c.parts.tobytes(), np.float32(c.score()).tobytes())


def _detect(model, im, dtype):
    from partsbaseddetector_amd import PartsBasedDetector
    det = PartsBasedDetector(device=0, dtype=dtype)
    det.distributeModel(model)
    out = det.detect(im)
    det.hd.close()
    return out


def _check(oracle, mat_model, xml_model, frames):
    seen = 0
    for seed, h, w, cn in frames:
        im = synth.synthetic_frame(seed, h, w, cn)
        for dtype in (np.float32, np.float64):
            got = _detect(mat_model, im, dtype)
            ref = _detect(xml_model, im, dtype)
            assert [_key(c) for c in got] == [_key(c) for c in ref], (seed, dtype)
            want = oracle.detect(xml_model.flatten(), im, dtype=dtype)
            assert len(got) == len(want), (seed, dtype, len(got), len(want))
            for g, o in zip(got, want):
                assert (g.level, g.component, g.root[1], g.root[0]) == (o["level"], o["component"], o["root_y"], o["root_x"])
                assert np.array_equal(g.parts, o["parts"])
                assert np.float32(g.score()) == np.float32(o["score"])
            seen += len(got)
    assert seen > 0


@pytest.mark.parametrize("which", ["v7", "v6", "be", "quirks"])
def test_fixture_detects_as_the_xml_model(oracle, which):
    mat = load_model_file(os.path.join(GOLDEN, f"matlab_fixture_{which}.mat"))
    _check(oracle, mat, load_model_file(XML), FRAMES)


def test_person_model_detects_as_the_xml_model(oracle, tmp_path):
    person = M.synthetic_person_model()
    mat, xml = str(tmp_path / "person.mat"), str(tmp_path / "person.xml")
    matlab_model.serialize(person, mat)
    filestorage.serialize_xml(person, xml)
    _check(oracle, load_model_file(mat), load_model_file(xml), [(4, 160, 200, 3), (5, 144, 176, 1)])


def test_demo_prints_the_same_for_mat_and_xml(tmp_path):
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    demo = os.path.join(ROOT, "host", "pbd_demo")
    im = synth.synthetic_frame(1, 96, 128, 3)
    ipath = str(tmp_path / "frame.ppm")
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())
    for flags in ([], ["--double"], ["--device-nms", "0.1", "--top", "5"]):
        want = subprocess.run([demo, XML, ipath] + flags, capture_output=True, text=True, timeout=300)
        assert want.returncode == 0, want.stderr
        assert "Number of candidates" in want.stdout and "cand " in want.stdout
        for which in ("v7", "quirks"):
            got = subprocess.run([demo, os.path.join(GOLDEN, f"matlab_fixture_{which}.mat"), ipath] + flags, capture_output=True,
                                 text=True, timeout=300)
            assert got.returncode == 0, got.stderr
            assert got.stdout == want.stdout, (which, flags)
