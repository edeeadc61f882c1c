"""The batch call of the reference-side binding (pbd_adapters::hipDetectBatch in include/pbd_opencv_adapters.hpp, over
pbd_bind.hpp's detect_batch) type-checks against the C ABI, for T = float and double, in every standard the adapters take.
Same method as tests/test_adapters_compile.py: g++ -fsyntax-only against the declarations in tests/adapter_doubles/."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")

TU = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipDetectBatch<float>(pbd_handle *, const vectorMat &, std::vector<vectorCandidate> &);
template void pbd_adapters::hipDetectBatch<double>(pbd_handle *, const vectorMat &, std::vector<vectorCandidate> &);
// what the reference's PartsBasedDetector<T>::detectBatch holds (INTEGRATION.md)
void detect_batch(pbd_adapters::Handle<double> &hip, const vectorMat &images, std::vector<vectorCandidate> &candidates)
{
    pbd_adapters::hipDetectBatch<double>(hip.h, images, candidates);
}
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_hip_detect_batch_compiles_against_the_c_abi(std, tmp_path):
    src = tmp_path / "batch_tu.cpp"
    src.write_text(TU)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_mirror_detect_batch_compiles(tmp_path):
    src = tmp_path / "host_tu.cpp"
    src.write_text('#include "pbd_host.hpp"\n'
                   'template class pbdhost::PartsBasedDetector<float>;\n'
                   'template class pbdhost::PartsBasedDetector<double>;\n')
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
