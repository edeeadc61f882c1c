"""The C++ host mirror's clusterParts (include/pbd_host.hpp) compiles without a GPU, for T = float and T = double, in C++11 and
C++17, and include/pbd.h's clustering declarations compile as C."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_cluster_member_compiles(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
double use(pbdhost::PartsBasedDetector<T> &d, const std::vector<double> &def)
{
    std::vector<int32_t> parent(3, 0), K(3, 2);
    parent[0] = -1;
    pbdhost::PartClusters c = d.clusterParts(def, parent, K);
    pbdhost::PartClusters e = d.clusterParts(def, parent, K, 8, 50, 7);
    return c.centres[0] + c.idx[0] + c.counts[0] + c.anchors[0] + c.info[0].best_trial + c.info[0].sumdist + e.sumdist_all[0] + e.iters_all[0];
}
template double use<float>(pbdhost::PartsBasedDetector<float> &, const std::vector<double> &);
template double use<double>(pbdhost::PartsBasedDetector<double> &, const std::vector<double> &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_declarations_compile_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('''
#include "pbd.h"
int use(pbd_handle *h, const double *def, const int32_t *parent, const int32_t *K, int32_t *i, double *c, struct pbd_cluster_info *info)
{
    return pbd_cluster_parts(h, 3, 8, def, parent, K, 100, 1000, 0, i, c, i, i, info, 0, 0)
         + pbd_cluster_parts_device(h, 3, 8, def, parent, K, 100, 1000, 0, i, c, i, i, info, c, i) + (int)sizeof(struct pbd_cluster_info);
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
