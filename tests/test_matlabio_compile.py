"""include/pbd_matlabio.hpp (pbdhost::MatlabIOModel) compiles on its own, warning-free, against pbd_host.hpp and zlib, and
links into a program that reads a committed .mat fixture -- no GPU, no OpenCV, no Boost."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
TU = ('#include "pbd_matlabio.hpp"\n#include <cstdio>\n'
      'int main(int argc, char **argv) {\n'
      '    pbdhost::MatlabIOModel m;\n    pbdhost::Model &base = m;\n'
      '    try { if (argc < 2 || !m.deserialize(argv[1])) return 1; }\n'
      '    catch (const pbdhost::Error &e) { std::printf("error %d %s\\n", e.code, e.what()); return 2; }\n'
      '    std::printf("%s %d %zu %d\\n", base.name().c_str(), base.ncomponents(), base.filtersw_.size(), base.flen());\n'
      '    return 0;\n}\n')


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_matlabio_header_compiles(tmp_path, std):
    src = tmp_path / "tu.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_matlabio_header_links_with_zlib_and_reads_a_fixture(tmp_path):
    src, exe = tmp_path / "tu.cpp", tmp_path / "tu"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", INCLUDE, str(src), "-o", str(exe), "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "matlab_fixture_v7.mat")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["matlab_fixture", "2", "8", "32"], (r.stdout, r.stderr)


def test_matlabio_header_is_opencv_free():
    text = open(os.path.join(INCLUDE, "pbd_matlabio.hpp")).read()
    assert "#include <opencv" not in text and "#include <boost" not in text
