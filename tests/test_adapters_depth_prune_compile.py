"""The depth-pruning calls of the reference-side binding (pbd_adapters::hipDepthPrune and hipSetDepthPrune in
include/pbd_opencv_adapters.hpp, over pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setDepthPrune / bindDepth /
depthPrune, FrameStream<T>::setDepthPrune and submit(im, depth) in include/pbd_host.hpp) type-check against the C ABI, in every
standard they take.  A function declared as include/SearchSpacePruning.hpp declares filterResponseByDepth forwards its arguments
to hipDepthPrune.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
namespace cv { struct Size { int width, height; }; }
static pbd_handle *g_h;
// include/SearchSpacePruning.hpp:56
template <typename T> struct SearchSpacePruning {
    void filterResponseByDepth(vector2DMat& pdfs, const std::vector<cv::Size>& fsizes, const cv::Mat& depth, const vectorf& scales, const float X, const float fx);
};
template <typename T>
void SearchSpacePruning<T>::filterResponseByDepth(vector2DMat& pdfs, const std::vector<cv::Size>& fsizes, const cv::Mat& depth, const vectorf& scales, const float X, const float fx)
{
    pbd_adapters::hipDepthPrune<T>(g_h, pdfs, fsizes, depth, scales, X, fx);
}
template struct SearchSpacePruning<float>;
template struct SearchSpacePruning<double>;
template void pbd_adapters::hipSetDepthPrune<float>(pbd_handle *, bool, float, float, float);
template void pbd_adapters::hipSetDepthPrune<double>(pbd_handle *, bool, float, float, float);
// what the reference's PartsBasedDetector<T>::detect holds in place of its commented-out calls (src/PartsBasedDetector.cpp:86-93)
void detect_with_depth(pbd_adapters::Handle<double> &hip, const cv::Mat &im, const cv::Mat &depth, vector2DMat &pdfs,
                       const std::vector<cv::Size> &fsizes, const vectorf &scales, vectorCandidate &candidates)
{
    pbd_adapters::hipDepthPrune<double>(hip.h, pdfs, fsizes, depth, scales, 0.5f, 525.f, 0.25f);
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    pbd_adapters::hipSetDepthPrune<double>(hip.h, false);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im, const pbdhost::Image &depth)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(bool, float, float, float) = &pbdhost::PartsBasedDetector<T>::setDepthPrune;
    (pbd.*set)(true, 525.f, 0.5f, 0.3f);
    pbd.setDepthPrune(true, 525.f, 0.5f);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, depth, c);
    pbd.bindDepth(depth);
    pbd.detect(im, c);
    pbd.depthPrune(depth, c, 525.f, 0.5f);
    pbd.depthPrune(depth, c, 525.f, 0.5f, 0.1f);
    pbd.setDepthPrune(false);
    pbdhost::FrameStream<T> fs(model, 2);
    fs.setDepthPrune(true, 525.f, 0.5f, 0.3f);
    fs.submit(im, depth);
    fs.next(c);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h, const pbd_frame *d, const int32_t *in, int32_t *out, int *n)
{
    pbd_depth_prune_cfg cfg = {525.f, 0.5f, 0.3f};
    return pbd_set_depth_prune(h, &cfg) + pbd_bind_depth(h, 1, d, 2) + pbd_bind_depth_device(h, 1, d, 5) +
           pbd_depth_prune(h, &cfg, 1, d, 2, in, 3, 0, out, 3, n) + pbd_depth_prune_device(h, &cfg, 1, d, 2, in, 3, 0, out, 3) +
           (PBD_K_DEPTH_PRUNE == PBD_K_COUNT - 1 ? 0 : 1);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "depth_prune_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "depth_prune_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "depth_prune_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
