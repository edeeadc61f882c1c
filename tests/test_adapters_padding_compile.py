"""The padded pyramid's calls of the reference-side binding (pbd_adapters::hipSetPadding in include/pbd_opencv_adapters.hpp, over
pbdbind::set_padding of pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setPadding and FrameStream<T>::setPadding
in include/pbd_host.hpp) type-check against the C ABI, in every standard they take, and pbd_set_padding of include/pbd.h compiles
as C.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipSetPadding<float>(pbd_handle *, int, int);
template void pbd_adapters::hipSetPadding<double>(pbd_handle *, int, int);
// people cut off by the frame edge, then the bare map again
void detect_past_the_edge(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &padded, vectorCandidate &bare)
{
    pbd_adapters::hipSetPadding<double>(hip.h, 2, 3);
    pbd_adapters::hipDetect<double>(hip.h, im, padded);
    pbd_adapters::hipSetPadding<double>(hip.h, 0, 0);
    pbd_adapters::hipDetect<double>(hip.h, im, bare);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(int, int) = &pbdhost::PartsBasedDetector<T>::setPadding;
    (pbd.*set)(2, 3);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    pbd.setPadding(0, 0);
    pbdhost::FrameStream<T> fs(model, 2);
    void (pbdhost::FrameStream<T>::*fset)(int, int) = &pbdhost::FrameStream<T>::setPadding;
    (fs.*fset)(2, 2);
    fs.submit(im);
    fs.next(c);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h)
{
    int (*set)(pbd_handle *, int, int) = pbd_set_padding;
    return set(h, 2, 3) + pbd_set_padding(h, 0, 0);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "padding_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "padding_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "padding_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
