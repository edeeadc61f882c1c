"""The grid NMS calls of the reference-side binding (pbd_adapters::hipGridNMS and hipSetRootNMS in include/pbd_opencv_adapters.hpp,
over pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setRootNMS / gridNMS, FrameStream<T>::setRootNMS in
include/pbd_host.hpp) type-check against the C ABI, in every standard they take.  A function declared as include/nms.hpp declares
nonMaximaSuppression forwards its arguments, default mask included, to hipGridNMS.  Same method as
tests/test_adapters_compile.py: g++ -fsyntax-only against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
// include/nms.hpp:42
void nonMaximaSuppression(const cv::Mat& src, const int sz, cv::Mat& dst, const cv::Mat mask=cv::Mat());
static pbd_handle *g_h;
void nonMaximaSuppression(const cv::Mat& src, const int sz, cv::Mat& dst, const cv::Mat mask) { pbd_adapters::hipGridNMS(g_h, src, sz, dst, mask); }
void (*const check_signature)(pbd_handle *, const cv::Mat &, int, cv::Mat &, const cv::Mat) = &pbd_adapters::hipGridNMS;
template void pbd_adapters::hipSetRootNMS<float>(pbd_handle *, int);
template void pbd_adapters::hipSetRootNMS<double>(pbd_handle *, int);
// what the reference's PartsBasedDetector<T>::detect holds in place of its commented-out call (src/PartsBasedDetector.cpp:86)
void detect_with_root_nms(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &candidates, cv::Mat &maxima)
{
    pbd_adapters::hipSetRootNMS<double>(hip.h, 2);
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    pbd_adapters::hipGridNMS(hip.h, im, 2, maxima);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(int) = &pbdhost::PartsBasedDetector<T>::setRootNMS;
    (pbd.*set)(2);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    pbdhost::MatT<T> plane(3, 4);
    std::vector<uint8_t> dst, mask(12, 1);
    pbd.gridNMS(plane, 1, dst);
    pbd.gridNMS(plane, 1, dst, mask);
    pbdhost::FrameStream<T> fs(model, 2);
    fs.setRootNMS(2);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "grid_nms_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "grid_nms_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
