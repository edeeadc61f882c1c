"""The part-score calls of the reference-side binding (pbd_adapters::hipPartScores in include/pbd_opencv_adapters.hpp, over
pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::partScores / scorePlacements in include/pbd_host.hpp) type-check
against the C ABI, in every standard they take, and the four declarations of include/pbd.h compile as C.  Same method as
tests/test_adapters_compile.py: g++ -fsyntax-only against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
// the confidence of every part of what was detected
double weakest_part(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &candidates)
{
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    std::vector<int32_t> status;
    std::vector<pbdbind::PartScore> scores;
    pbd_adapters::hipPartScores<double>(hip.h, candidates, status, scores);
    double low = 0;
    for (size_t j = 0; j < scores.size(); ++j) low = scores[j].appearance < low ? scores[j].appearance : low;
    return low + scores[0].message + scores[0].bias + scores[0].total + scores[0].x + scores[0].y + scores[0].m + status[0];
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c;
    pbd.detect(im, c);
    std::vector<pbdhost::PartScore> scores, again;
    pbd.partScores(c, scores);
    std::vector<int32_t> status;
    pbd.scorePlacements(c, scores, status, again);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h, const int32_t *rec, int32_t *status, int32_t *place, float *scores)
{
    return pbd_part_scores(h, rec, 4, 0, status, place, scores) + pbd_part_scores(h, rec, 4, 0, status, 0, scores) +
           pbd_part_scores_device(h, rec, 4, 0, status, place, scores) + pbd_score_placements(h, rec, 4, 0, place, status, scores) +
           pbd_score_placements_device(h, rec, 4, 0, place, status, scores);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_call_compiles_against_the_c_abi(std, tmp_path):
    src = tmp_path / "part_scores_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "part_scores_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "part_scores_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
