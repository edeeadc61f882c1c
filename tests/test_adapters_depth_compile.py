"""The depth-consistency and suppression calls of the reference-side binding (pbd_adapters::hipFilterCandidatesByDepth and
hipSuppress in include/pbd_opencv_adapters.hpp, over pbd_bind.hpp) type-check against the C ABI, for T = float and double, in
every standard the adapters take.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against declarations
(tests/adapter_doubles_depth/ adds the Candidate accessors these calls read)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipFilterCandidatesByDepth<float>(pbd_handle *, vectorCandidate &, const cv::Mat &, float);
template void pbd_adapters::hipFilterCandidatesByDepth<double>(pbd_handle *, vectorCandidate &, const cv::Mat &, float);
template void pbd_adapters::hipSuppress<float>(pbd_handle *, const cv::Mat &, vectorCandidate &, float);
template void pbd_adapters::hipSuppress<double>(pbd_handle *, const cv::Mat &, vectorCandidate &, float);
// what the reference's PartsBasedDetector<T>::detect(im, depth, candidates) holds in place of its commented-out call, followed
// by the callers' sort + suppression (cells/detect.cpp:237-238)
void detect_tail(pbd_adapters::Handle<double> &hip, const cv::Mat &im, const cv::Mat &depth, vectorCandidate &candidates)
{
    pbd_adapters::hipFilterCandidatesByDepth<double>(hip.h, candidates, depth, 0.03f);
    pbd_adapters::hipSuppress<double>(hip.h, im, candidates, 0.1f);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_depth_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "depth_tu.cpp"
    src.write_text(TU)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
