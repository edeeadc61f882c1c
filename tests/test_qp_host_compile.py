"""The C++ host mirror's training QP (include/pbd_host.hpp pbdhost::QP, PartsBasedDetector::qp) compiles without a GPU, for
T = float and T = double, in C++11 and C++17."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_qp_members_compile(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
double use(pbdhost::PartsBasedDetector<T> &d, const std::vector<pbdhost::Candidate> &c)
{
    std::vector<int32_t> hdr;
    std::vector<T> values;
    int hdr_words = 0, nvalues = 0;
    d.examples(c, hdr, values, hdr_words, nvalues);
    pbdhost::QP q = d.qp(1000, 0.002, 2.0);
    std::vector<int32_t> ids(5 * c.size(), 1);
    int taken = q.add(d.handle(), hdr, values, ids);
    q.fix();
    int n = q.prune();
    pbd_qp_info s = q.one(std::vector<int32_t>(), 7);
    s = q.opt(0.05, 100, 1);
    pbdhost::QP moved(std::move(q));
    std::vector<double> w = moved.weights(), sc = moved.scores();
    return w[0] + sc.size() + taken + n + s.lb + moved.state().ub;
}
template double use<float>(pbdhost::PartsBasedDetector<float> &, const std::vector<pbdhost::Candidate> &);
template double use<double>(pbdhost::PartsBasedDetector<double> &, const std::vector<pbdhost::Candidate> &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
