"""pbdhost::MatlabIOModel (include/pbd_matlabio.hpp) through host/pbd_demo, which chooses the model reader by extension as
the reference's demo does (src/demo.cpp:63-77).  `--dump-model` needs no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import filestorage, matlab_model
from partsbaseddetector_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEMO = os.path.join(ROOT, "host", "pbd_demo")
XML = os.path.join(GOLDEN, "matlab_fixture.xml")


@pytest.fixture(scope="module")
def demo():
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return DEMO


def _dump(demo, path):
    r = subprocess.run([demo, path, "--dump-model"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("which", ["v7", "v6", "be", "quirks"])
def test_dump_model_mat_equals_xml(demo, which):
    got = _dump(demo, os.path.join(GOLDEN, f"matlab_fixture_{which}.mat"))
    assert got == _dump(demo, XML)
    assert got.startswith("name matlab_fixture\ninterval 5\n") and "part 1 2 parent 0 filterid 7 biasid 12 13 defid 6" in got


@pytest.mark.parametrize("compress", [True, False])
def test_dump_model_of_written_models(demo, tmp_path, compress):
    """models written by matlab_model.serialize, person-sized included: the C++ reader reads what the Python one does"""
    for i, m in enumerate([M.synthetic_person_model(), M.synthetic_face_model(thresh=1.5, nparts=7, ncomponents=2)]):
        mat, xml = str(tmp_path / f"m{i}.mat"), str(tmp_path / f"m{i}.xml")
        matlab_model.serialize(m, mat, compress=compress)
        filestorage.serialize_xml(matlab_model.deserialize(mat), xml)
        assert _dump(demo, mat) == _dump(demo, xml)


def _fails_cleanly(demo, path):
    r = subprocess.run([demo, path, "--dump-model"], capture_output=True, text=True, timeout=60)
    assert r.returncode > 0, (r.returncode, r.stderr)            # an exit status, not a signal
    assert r.stderr.strip(), "no message"
    return r


@pytest.mark.parametrize("which", ["v7", "v6", "be", "quirks"])
def test_corrupt_or_truncated_mat_fails_with_a_message(demo, tmp_path, which):
    raw = open(os.path.join(GOLDEN, f"matlab_fixture_{which}.mat"), "rb").read()
    p = str(tmp_path / "bad.mat")
    rng = np.random.default_rng(len(raw))
    for cut in [0, 2, 64, 127, 128, 131, 140, 200, 1000] + sorted(rng.integers(129, len(raw) - 8, 12).tolist()):
        open(p, "wb").write(raw[:cut])
        _fails_cleanly(demo, p)
    # lengths and dimensions rewritten to huge values
    big = bytearray(raw)
    struct.pack_into("<I" if which != "be" else ">I", big, 132, 0x7FFFFFF0)
    open(p, "wb").write(bytes(big))
    _fails_cleanly(demo, p)
    # random bytes overwritten: an error or a model, never a crash
    for k in range(40):
        b = bytearray(raw)
        for i in rng.integers(128, len(raw), 3):
            b[i] = int(rng.integers(0, 256))
        open(p, "wb").write(bytes(b))
        r = subprocess.run([demo, p, "--dump-model"], capture_output=True, text=True, timeout=60)
        assert r.returncode >= 0 and (r.returncode == 0 or r.stderr.strip()), (k, r.returncode, r.stderr)


def test_v73_and_level4_are_refused(demo, tmp_path):
    p = tmp_path / "v73.mat"
    head = b"MATLAB 7.3 MAT-file, Platform: GLNXA64, Created on: Mon Jan  1 00:00:00 2024 HDF5 schema 1.00 .".ljust(116, b" ")
    p.write_bytes(head + b"\0" * 8 + struct.pack("<H", 0x0200) + b"IM" + b"\0" * 384 + b"\x89HDF\r\n\x1a\n" + b"\0" * 64)
    assert "save -v7" in _fails_cleanly(demo, str(p)).stderr
    p.write_bytes(struct.pack("<5i", 0, 1, 1, 0, 9) + b"interval\0" + struct.pack("<d", 5.0))
    assert "level 4" in _fails_cleanly(demo, str(p)).stderr


def test_missing_field_is_named(demo, tmp_path):
    from partsbaseddetector_amd import matio
    d = matio.loadmat(os.path.join(GOLDEN, "matlab_fixture_v7.mat"))
    for part in d["model"][0]["components"][1]:
        part.pop("biasid")
    d["model"][0]["components"][1].fieldnames.remove("biasid")
    p = str(tmp_path / "m.mat")
    matio.savemat(p, d)
    assert "missing field model.components{2}(1).biasid" in _fails_cleanly(demo, p).stderr
