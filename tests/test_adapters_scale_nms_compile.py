"""The scale-NMS calls of the reference-side binding (pbd_adapters::hipSetScaleNMS and hipScaleNMS in
include/pbd_opencv_adapters.hpp, over pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setScaleNMS / scaleNMS and
FrameStream<T>::setScaleNMS in include/pbd_host.hpp) type-check against the C ABI, in every standard they take, and the three
declarations and the enumerator of include/pbd.h compile as C.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only
against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipSetScaleNMS<float>(pbd_handle *, bool, int);
template void pbd_adapters::hipSetScaleNMS<double>(pbd_handle *, bool, int);
// five distinct people per image, then a list built elsewhere
void detect_distinct(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &candidates)
{
    pbd_adapters::hipSetScaleNMS<double>(hip.h, true, 2);
    pbd_adapters::hipSetTopK<double>(hip.h, 5);
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    pbd_adapters::hipSetScaleNMS<double>(hip.h, false, 0);
    pbd_adapters::hipScaleNMS<double>(hip.h, candidates, 5);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(bool, int) = &pbdhost::PartsBasedDetector<T>::setScaleNMS;
    (pbd.*set)(true, 2);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    pbd.scaleNMS(c, 5);
    pbd.setScaleNMS(false);
    pbdhost::FrameStream<T> fs(model, 2);
    fs.setScaleNMS(true, 1);
    fs.submit(im);
    fs.next(c);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h, const int32_t *in, int32_t *out, int *n)
{
    return pbd_set_scale_nms(h, 1, 2) + pbd_scale_nms(h, 1, 2, in, 4, 0, out, 4, n) + pbd_scale_nms_device(h, 1, 2, in, 4, 0, out, 4) +
           (PBD_K_SCALE_NMS == PBD_K_MM_DECODE + 1 && PBD_K_SCALE_NMS == PBD_K_COUNT - 1 ? 0 : 1);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "scale_nms_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "scale_nms_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "scale_nms_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
