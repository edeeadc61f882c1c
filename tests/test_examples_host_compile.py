"""The C++ host mirror's training-example members (include/pbd_host.hpp modelVector, examples, detectLatent) compile without a GPU, for
T = float and T = double, in C++11 and C++17."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_example_members_compile(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
size_t use(pbdhost::PartsBasedDetector<T> &d, const std::vector<pbdhost::Candidate> &c)
{
    std::vector<T> w = d.modelVector();
    std::vector<int32_t> hdr;
    std::vector<T> values;
    int hdr_words = 0, nvalues = 0;
    d.examples(c, hdr, values, hdr_words, nvalues);
    std::vector<pbdhost::Image> ims(1);
    std::vector<std::vector<int32_t> > boxes(1, std::vector<int32_t>(12, 0)), mix;
    std::vector<pbdhost::Candidate> pos;
    std::vector<bool> found;
    d.detectLatent(ims, boxes, 0.5f, mix, pos, found);
    return w.size() + hdr.size() + values.size() + (size_t)hdr_words + (size_t)nvalues;
}
template size_t use<float>(pbdhost::PartsBasedDetector<float> &, const std::vector<pbdhost::Candidate> &);
template size_t use<double>(pbdhost::PartsBasedDetector<double> &, const std::vector<pbdhost::Candidate> &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
