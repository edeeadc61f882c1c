"""The C++ host mirror's additions for training (include/pbd_host.hpp: PartsBasedDetector::setWalk, pbdhost::QP::clear and
addLoss) compile without a GPU, for T = float and T = double, in C++11 and C++17."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_train_members_compile(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
double use(pbdhost::PartsBasedDetector<T> &d, const int32_t *d_payload, int capacity)
{
    d.setWalk(PBD_WALK_ARGMAX);
    pbdhost::QP q = d.qp(1000, 0.002, 2.0);
    q.clear();
    double added = q.addLoss(d_payload, capacity) + q.addLoss(d_payload, capacity, 1);
    d.setWalk(PBD_WALK_REFERENCE);
    int rc = pbd_set_walk(d.handle(), PBD_WALK_ARGMAX) + pbd_qp_clear(q.get())
           + pbd_qp_add_loss_device(q.get(), d_payload, capacity, -1, NULL);
    return added + rc + q.state().ub;
}
template double use<float>(pbdhost::PartsBasedDetector<float> &, const int32_t *, int);
template double use<double>(pbdhost::PartsBasedDetector<double> &, const int32_t *, int);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
