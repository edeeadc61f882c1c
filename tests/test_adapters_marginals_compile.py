"""The max-marginal calls of the reference-side binding (pbd_adapters::hipMaxMarginals / hipMarginalPoses in
include/pbd_opencv_adapters.hpp, over pbd_bind.hpp) and of the host mirror (PartsBasedDetector<T>::maxMarginals / marginalPoses in
include/pbd_host.hpp) type-check against the C ABI, in every standard they take, and the five declarations of include/pbd.h
compile as C.  Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against declarations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")

TU_ADAPTERS = """#include "pbd_opencv_adapters.hpp"
// the pose with part 3 at its best cell of level 0
double best_of_part(pbd_adapters::Handle<double> &hip, const cv::Mat &im, vectorCandidate &candidates, int planes)
{
    pbd_adapters::hipDetect<double>(hip.h, im, candidates);
    std::vector<pbdbind::MarginalLevel> levels;
    pbd_adapters::hipMaxMarginals<double>(hip.h, 0, im.rows, im.cols, planes, levels);
    std::vector<int32_t> seeds(6, 0), status;
    seeds[2] = 3; seeds[3] = -1;
    vectorCandidate poses;
    pbd_adapters::hipMarginalPoses<double>(hip.h, seeds, status, poses);
    return levels[0].values[0] + levels[0].rows + levels[0].cols + levels[0].planes + status[0] + (double)poses.size();
}
"""

TU_HOST = """#include "pbd_host.hpp"
template <typename T> void use(pbdhost::Model &model, const pbdhost::Image &im)
{
    pbdhost::PartsBasedDetector<T> pbd;
    pbd.distributeModel(model);
    std::vector<pbdhost::Candidate> c, poses;
    pbd.detect(im, c);
    std::vector<pbdhost::MarginalLevel> levels;
    pbd.maxMarginals(im, levels);
    pbd.maxMarginals(im, levels, 0);
    std::vector<int32_t> seeds(6, 0), status;
    pbd.marginalPoses(seeds, status, poses);
}
template void use<float>(pbdhost::Model &, const pbdhost::Image &);
template void use<double>(pbdhost::Model &, const pbdhost::Image &);
"""

TU_C = """#include "pbd.h"
int use(pbd_handle *h, const int32_t *seeds, const float *scales, int32_t *cand, int32_t *place, int32_t *status, float *dst)
{
    void *d = 0;
    return pbd_max_marginals(h, 0) + pbd_get_marginals(h, 0, PBD_MM_VALUES, dst, 16) + pbd_get_marginals(h, 0, PBD_MM_PARENT_K, dst, 16) +
           pbd_marginals_device(h, 0, &d) + pbd_marginal_poses(h, 2, seeds, scales, 0, cand, place, status) +
           pbd_marginal_poses(h, 2, seeds, 0, 0, cand, 0, status) + pbd_marginal_poses_device(h, 2, seeds, scales, 0, cand, place, status) +
           (PBD_K_MM_DT_ROWS < PBD_K_MM_DECODE && PBD_K_MM_DECODE < PBD_K_COUNT ? 0 : 1);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "marginals_tu.cpp"
    src.write_text(TU_ADAPTERS)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_mirror_calls_compile(std, tmp_path):
    src = tmp_path / "marginals_host_tu.cpp"
    src.write_text(TU_HOST)
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "marginals_c.c"
    src.write_text(TU_C)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
