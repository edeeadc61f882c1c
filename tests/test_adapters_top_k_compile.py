"""The top-K calls of the reference-side binding (pbd_adapters::hipTopK, both forms, and hipSetTopK in
include/pbd_opencv_adapters.hpp, over pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::setTopK / topKCells / topK and
FrameStream<T>::setTopK in include/pbd_host.hpp) type-check against the C ABI, in every standard they take, and the five
declarations and the enumerator of include/pbd.h compile as C.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only
against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipSetTopK<float>(pbd_handle *, int);
template void pbd_adapters::hipSetTopK<double>(pbd_handle *, int);
// at most five people per image, then the best one of a list built elsewhere
void detect_the_best(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &candidates, const cv::Mat &scores,
                     const cv::Mat &mask, cv::Mat &best)
{
    pbd_adapters::hipSetTopK<double>(hip.h, 5);
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    pbd_adapters::hipSetTopK<double>(hip.h, 0);
    pbd_adapters::hipTopK<double>(hip.h, candidates, 1);
    pbd_adapters::hipTopK(hip.h, scores, 3, best);
    pbd_adapters::hipTopK(hip.h, scores, 3, best, mask);
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im, const pbdhost::MatT<T> &scores)
{
    pbdhost::PartsBasedDetector<T> pbd;
    void (pbdhost::PartsBasedDetector<T>::*set)(int) = &pbdhost::PartsBasedDetector<T>::setTopK;
    (pbd.*set)(5);
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    pbd.topK(c, 1);
    std::vector<uint8_t> dst, mask;
    pbd.topKCells(scores, 3, dst);
    pbd.topKCells(scores, 3, dst, mask);
    pbd.setTopK(0);
    pbdhost::FrameStream<T> fs(model, 2);
    fs.setTopK(5);
    fs.submit(im);
    fs.next(c);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &, const pbdhost::MatT<float> &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &, const pbdhost::MatT<double> &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h, const long long *len, const float *src, const uint8_t *mask, uint8_t *dst, const int32_t *in, int32_t *out, int *n)
{
    return pbd_set_top_k(h, 5) + pbd_top_k_cells(h, 2, len, PBD_REAL_F32, src, mask, 3, dst) +
           pbd_top_k_cells_device(h, 2, len, PBD_REAL_F64, src, 0, 3, dst) + pbd_top_k(h, 1, 3, in, 4, 0, out, 4, n) +
           pbd_top_k_device(h, 1, 3, in, 4, 0, out, 4) +
           (PBD_K_TOP_K == PBD_K_GRID_NMS + 1 && PBD_K_DEPTH_PRUNE == PBD_K_TOP_K + 1 && PBD_K_DEPTH_PRUNE == PBD_K_COUNT - 1 ? 0 : 1);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "top_k_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "top_k_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "top_k_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
