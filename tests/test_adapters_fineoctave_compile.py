"""The fine octave's calls of the reference-side binding (pbd_adapters::hipSetFineOctave in include/pbd_opencv_adapters.hpp, over
pbdbind::set_fine_octave of pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setFineOctave and
FrameStream<T>::setFineOctave in include/pbd_host.hpp) type-check against the C ABI, in every standard they take, and
pbd_set_fine_octave of include/pbd.h compiles as C.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against
declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipSetFineOctave<float>(pbd_handle *, bool);
template void pbd_adapters::hipSetFineOctave<double>(pbd_handle *, bool);
// people at the far end of the room, then the reference's own levels again
void detect_small_objects(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &fine, vectorCandidate &bare)
{
    pbd_adapters::hipSetFineOctave<double>(hip.h, true);
    pbd_adapters::hipSetPadding<double>(hip.h, 2, 2);
    pbd_adapters::hipDetect<double>(hip.h, im, fine);
    pbd_adapters::hipSetFineOctave<double>(hip.h, false);
    pbd_adapters::hipDetect<double>(hip.h, im, bare);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(bool) = &pbdhost::PartsBasedDetector<T>::setFineOctave;
    (pbd.*set)(true);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    pbd.setFineOctave(false);
    pbdhost::FrameStream<T> fs(model, 2);
    void (pbdhost::FrameStream<T>::*fset)(bool) = &pbdhost::FrameStream<T>::setFineOctave;
    (fs.*fset)(true);
    fs.submit(im);
    fs.next(c);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h)
{
    int (*set)(pbd_handle *, int) = pbd_set_fine_octave;
    return set(h, 1) + pbd_set_fine_octave(h, 0);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "fineoctave_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "fineoctave_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "fineoctave_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
