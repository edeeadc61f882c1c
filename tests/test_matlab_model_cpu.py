"""Models saved by the Matlab training code (.mat, level 5): the MAT reader (partsbaseddetector_amd/matio.py), the model
layout (matlab_model.py), the writer, the converter and the extension-chosen loader.  No GPU.

The fixtures (tests/golden/make_matlab_fixtures.py) were written by scipy.io.savemat, transcoded to big-endian, or typed
out element by element; tests/golden/matlab_fixture.xml is the same model as filestorage.serialize_xml writes it."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from partsbaseddetector_amd import config, filestorage, load_model_file, matio, matlab_model
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.matio import MatCell, MatStruct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["v7", "v6", "be", "quirks"]
FIELDS = ["name", "interval", "thresh", "sbin", "norient", "flen", "biasw", "anchors", "defw", "filterid", "biasid", "defid", "parentid"]


def _mat(which):
    return os.path.join(GOLDEN, f"matlab_fixture_{which}.mat")


XML = os.path.join(GOLDEN, "matlab_fixture.xml")


def assert_same_model(got, want):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a == b and type(a) is type(b), (f, a, b)
    assert len(got.filtersw) == len(want.filtersw)
    for a, b in zip(got.filtersw, want.filtersw):
        assert a.dtype == np.float64 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("which", FIXTURES)
def test_fixture_equals_the_xml_model(which):
    assert_same_model(matlab_model.deserialize(_mat(which)), filestorage.deserialize(XML))


@pytest.mark.parametrize("which", FIXTURES)
def test_load_model_file_chooses_by_extension(which):
    assert_same_model(load_model_file(_mat(which)), load_model_file(XML))


def test_fixture_layout_quirks_are_present():
    """the hand-typed fixture really holds what scipy does not write"""
    raw = open(_mat("quirks"), "rb").read()
    assert struct.pack("<II", 14, 0) in raw                     # zero-byte miMATRIX
    assert struct.pack("<HH", 2, 1) in raw                      # small miUINT8 element (a double scalar)
    assert "Grüße".encode("utf-8") in raw                       # miUTF8 text
    d = matio.loadmat(_mat("quirks"))
    assert d["notes"][1] == "Grüße – été" and d["notes"][0].shape == (0, 0)
    assert open(_mat("be"), "rb").read()[126:128] == b"MI"
    assert open(_mat("v7"), "rb").read()[128] == 15             # miCOMPRESSED


# ------------------------------------------------------------------------------------------ reader vs scipy
def _ours(v):
    if isinstance(v, str):
        return ("str", v)
    if isinstance(v, MatCell):
        return ("cell", tuple(v.shape), [_ours(x) for x in v])
    if isinstance(v, MatStruct):
        return ("struct", tuple(v.shape), list(v.fieldnames), [[_ours(e[f]) for f in v.fieldnames] for e in v])
    assert isinstance(v, np.ndarray)
    return _num(v)


def _num(a):
    if a.size == 0:
        return ("empty",)                                        # a zero-byte miMATRIX: scipy gives (1, 0), Matlab []
    kind = "bool" if a.dtype == np.bool_ else a.dtype.str[1:]
    return ("num", a.shape, kind, a.astype(np.float64).ravel(order="F").tolist() if kind != "bool" else a.ravel(order="F").tolist())


def _theirs(v):
    if isinstance(v, np.ndarray) and v.dtype.kind == "U":
        return ("str", "".join(v.ravel().tolist()))
    if isinstance(v, np.ndarray) and v.dtype.names:
        flat = v.ravel(order="F")
        return ("struct", v.shape, list(v.dtype.names), [[_theirs(e[f]) for f in v.dtype.names] for e in flat])
    if isinstance(v, np.ndarray) and v.dtype == object:
        return ("cell", v.shape, [_theirs(x) for x in v.ravel(order="F")])
    return _num(v)


def _normalise_logical(t):
    """scipy returns logical arrays as bool or uint8 depending on version: compare them as bool"""
    if isinstance(t, tuple) and t and t[0] == "num" and t[2] == "u1":
        return ("num", t[1], "bool?", [bool(x) for x in t[3]])
    if isinstance(t, tuple) and t and t[0] == "num" and t[2] == "bool":
        return ("num", t[1], "bool?", t[3])
    if isinstance(t, tuple):
        return tuple(_normalise_logical(x) for x in t)
    if isinstance(t, list):
        return [_normalise_logical(x) for x in t]
    return t


def _assert_matches_scipy(path):
    sio = pytest.importorskip("scipy.io")
    want = {k: v for k, v in sio.loadmat(path, squeeze_me=False, mat_dtype=True).items() if not k.startswith("__")}
    got = matio.loadmat(path)
    assert list(got) == list(want)
    for k in want:
        a, b = _ours(got[k]), _theirs(want[k])
        if a != b:
            assert _normalise_logical(a) == _normalise_logical(b), k


@pytest.mark.parametrize("which", FIXTURES)
def test_reader_matches_scipy_on_fixtures(which):
    _assert_matches_scipy(_mat(which))


def _random_value(rng, depth):
    kind = rng.integers(0, 9 if depth < 3 else 6)
    if kind == 0:
        return "".join(chr(c) for c in rng.integers(32, 0x3000, rng.integers(0, 7)))
    if kind <= 5:
        dt = rng.choice(["f8", "f4", "i1", "u1", "i2", "u2", "i4", "u4", "i8", "u8", "bool"])
        shape = tuple(int(s) for s in rng.integers(0, 4, rng.integers(2, 4)))
        if dt == "bool":
            return rng.integers(0, 2, shape).astype(bool)
        if dt[0] == "f":
            return (rng.standard_normal(shape) * 100).astype(dt)
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    if kind <= 6:
        c = np.empty((1, int(rng.integers(1, 4))), dtype=object)
        for i in range(c.size):
            c[0, i] = _random_value(rng, depth + 1)
        return c
    names = ["alpha", "b", "w", "filterid", "z9"][:int(rng.integers(1, 6))]
    n = int(rng.integers(1, 4))
    s = np.empty((n, 1) if rng.integers(0, 2) else (1, n), dtype=[(f, object) for f in names])
    for e in s.ravel():
        for f in names:
            e[f] = _random_value(rng, depth + 1)
    return s


@pytest.mark.parametrize("seed", range(50))
def test_reader_matches_scipy_on_random_documents(tmp_path, seed):
    sio = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(seed)
    doc = {f"v{i}": _random_value(rng, 0) for i in range(int(rng.integers(1, 5)))}
    path = str(tmp_path / "doc.mat")
    sio.savemat(path, doc, do_compression=bool(seed % 2), format="5", oned_as="row")
    _assert_matches_scipy(path)


def test_writer_output_is_what_scipy_reads(tmp_path):
    sio = pytest.importorskip("scipy.io")
    path = str(tmp_path / "w.mat")
    doc = {"s": "text", "a": np.arange(24, dtype=np.int16).reshape(2, 3, 4), "l": np.array([[True, False]]), "e": np.zeros((0, 3)),
           "c": MatCell(["x", np.float32(2.5), MatCell([], (0, 0))], (3, 1)),
           "st": MatStruct([{"p": 1.0, "q": "r"}, {"p": np.array([[1.0, 2.0]]), "q": ""}], ["q", "p"], (2, 1))}
    for compress in (False, True):
        matio.savemat(path, doc, compress=compress)
        _assert_matches_scipy(path)
        got = matio.loadmat(path)
        assert got["s"] == "text" and got["a"].dtype == np.int16 and np.array_equal(got["a"], doc["a"])
        assert got["st"].fieldnames == ["q", "p"] and got["st"].shape == (2, 1) and got["st"][1]["p"].tolist() == [[1.0, 2.0]]
    assert sio.loadmat(path)["a"][1, 2, 3] == 23


# ------------------------------------------------------------------------------------------ writer, converter, config
def _models():
    base = filestorage.deserialize(XML)
    out = [base]
    for m in (M.synthetic_face_model(thresh=1.5, nparts=7, ncomponents=2), M.synthetic_tiny_model(thresh=0.25)):
        m.biasw = [float(np.float32(b)) for b in m.biasw]         # what a float model file holds (vector<float> in the reference)
        m.defw = [[float(np.float32(v)) for v in d] for d in m.defw]
        out.append(m)
    return out


@pytest.mark.parametrize("compress", [True, False])
def test_serialize_deserialize_is_the_identity(tmp_path, compress):
    for i, m in enumerate(_models()):
        path = str(tmp_path / f"m{i}.mat")
        assert matlab_model.serialize(m, path, compress=compress)
        assert (open(path, "rb").read()[128] == 15) == compress
        assert_same_model(matlab_model.deserialize(path), m)


def _transfer(src, dst):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "partsbaseddetector_amd.model_transfer", src, dst], capture_output=True, text=True,
                          cwd=ROOT, env=env, timeout=120)


def test_model_transfer_mat_xml_mat(tmp_path):
    xml, yml, mat = str(tmp_path / "a.xml"), str(tmp_path / "b.yml"), str(tmp_path / "c.mat")
    r = _transfer(_mat("v7"), xml)
    assert r.returncode == 0, r.stderr
    r = _transfer(xml, mat)
    assert r.returncode == 0, r.stderr
    r = _transfer(mat, yml)
    assert r.returncode == 0, r.stderr
    want = filestorage.deserialize(XML)
    for p in (xml, mat, yml):
        assert_same_model(load_model_file(p), want)
    r = _transfer(mat, str(tmp_path / "d.bin"))
    assert r.returncode != 0 and "unsupported model format" in r.stderr


def test_load_model_file_refuses_other_extensions(tmp_path):
    p = tmp_path / "model.txt"
    p.write_text(open(XML).read())
    with pytest.raises(ValueError, match="unsupported model format"):
        load_model_file(str(p))


def test_config_loads_a_mat_model(tmp_path):
    conf = tmp_path / "c.by_parts"
    conf.write_text("pipe:\n  type: PartsBasedDetector\n  parameters:\n    extra:\n"
                    f"      model_file: /nowhere/matlab_fixture_quirks.mat\n")
    cfg = config.load_by_parts(str(conf))[0]
    assert_same_model(config.load_model(cfg, search_dirs=[GOLDEN]), filestorage.deserialize(XML))


# ------------------------------------------------------------------------------------------ refusals
def test_v73_file_is_refused(tmp_path):
    head = b"MATLAB 7.3 MAT-file, Platform: GLNXA64, Created on: Mon Jan  1 00:00:00 2024 HDF5 schema 1.00 .".ljust(116, b" ")
    p = tmp_path / "v73.mat"
    p.write_bytes(head + b"\0" * 8 + struct.pack("<H", 0x0200) + b"IM" + b"\0" * 384 + b"\x89HDF\r\n\x1a\n" + b"\0" * 64)
    with pytest.raises(ValueError, match="v7.3.*save -v7"):
        matlab_model.deserialize(str(p))


def test_level4_file_is_refused(tmp_path):
    sio = pytest.importorskip("scipy.io")
    p = str(tmp_path / "v4.mat")
    sio.savemat(p, {"interval": np.array([[5.0]])}, format="4")
    with pytest.raises(ValueError, match="level 4.*save -v7"):
        matio.loadmat(p)


def test_sparse_and_complex_are_refused(tmp_path):
    sio = pytest.importorskip("scipy.io")
    sparse = pytest.importorskip("scipy.sparse")
    p = str(tmp_path / "x.mat")
    sio.savemat(p, {"ok": np.ones((1, 2)), "sp": sparse.csc_matrix(np.eye(3))})
    with pytest.raises(ValueError, match="'sp'.*sparse"):
        matio.loadmat(p)
    sio.savemat(p, {"cx": np.array([[1 + 2j]])})
    with pytest.raises(ValueError, match="'cx'.*complex"):
        matio.loadmat(p)


def test_missing_field_is_named_by_its_path(tmp_path):
    m = filestorage.deserialize(XML)
    p = str(tmp_path / "m.mat")
    matlab_model.serialize(m, p)
    d = matio.loadmat(p)
    comp = d["model"][0]["components"][1]
    for part in comp:
        part.pop("defid")
    comp.fieldnames.remove("defid")
    matio.savemat(p, d)
    with pytest.raises(ValueError, match=r"missing field model\.components\{2\}\(1\)\.defid"):
        matlab_model.deserialize(p)
    d["model"][0].pop("sbin")
    d["model"].fieldnames.remove("sbin")
    matio.savemat(p, d)
    with pytest.raises(ValueError, match=r"missing field model\.sbin"):
        matlab_model.deserialize(p)


def test_name_falls_back_to_the_file_stem(tmp_path):
    d = matio.loadmat(_mat("v7"))
    del d["name"]
    p = str(tmp_path / "person_model.mat")
    matio.savemat(p, d)
    assert matlab_model.deserialize(p).name == "person_model"


@pytest.mark.parametrize("which", FIXTURES)
def test_truncated_files_raise_value_error(tmp_path, which):
    raw = open(_mat(which), "rb").read()
    p = tmp_path / "t.mat"
    for cut in (0, 3, 100, 130, 200, len(raw) // 2, len(raw) - 9):
        p.write_bytes(raw[:cut])
        with pytest.raises(ValueError):
            matlab_model.deserialize(str(p))
