"""The weight layouts' one definition (partsbaseddetector_amd/csrc/pbd_layout.h), shared by the host packer of pbd_create and the
in-place model update's kernels, checked without a GPU through a small host-only build: every layout function maps the
destination index range onto the source values with padding as the only unmapped slots, and packing a random bank through it
equals a plain re-statement of the documented layout.  Also: include/pbd_host.hpp's update methods compile on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")

SRC = r'''
#include "pbd_layout.h"
using namespace pbd;
// out[i] = {filter, tap, channel, part} of destination i
extern "C" {
void map_generic(long long n, int KK, int Fpad, int nf, int *out)
{ for (long long i = 0; i < n; ++i) { WeightSrc s = generic_bank_source(i, KK, Fpad, nf); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = 0; } }
void map_group(long long n, int KK, int nf, int *out)
{ for (long long i = 0; i < n; ++i) { WeightSrc s = group_bank_source(i, KK, nf); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = 0; } }
void map_unit(long long n, int KK, int f0, int ql, int nf, int *out)
{ for (long long i = 0; i < n; ++i) { WeightSrc s = unit_source(i, KK, f0, ql, nf); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = 0; } }
void map_frag64(long long n, int KK, int QN, int mtiles, int passes, int nf, int *out)
{ for (long long i = 0; i < n; ++i) { WeightSrc s = f64_frag_source(i, KK, QN, mtiles, passes, nf); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = 0; } }
void map_wrec(long long n, int KK, int NV, int nfilters, int *out)
{ for (long long i = 0; i < n; ++i) { int part = 0; WeightSrc s = wrec_source(i, KK, NV, nfilters, &part); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = part; } }
long long size_generic(int KK, int Fpad) { return generic_bank_size(KK, Fpad); }
long long size_unit(int KK, int ql) { return unit_size(KK, ql); }
long long size_frag64(int KK, int mtiles) { return f64_frag_size(KK, mtiles); }
long long size_wrec(int KK, int NV, int nfilters) { return wrec_size(KK, NV, nfilters); }
int pass_begin(int ps, int mtiles, int passes) { return mfma_pass_begin(ps, mtiles, passes); }
int tap_outside(int cs, int i, int j) { return c31_tap_outside(cs, i, j) ? 1 : 0; }
unsigned value16(float v, int f16, int part) { return wrec_value(v, f16 != 0, part); }
int weight_place(int t, int c) { WeightSrc s = {0, t, c}; return weight_at(s); }
}
'''


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout")
    src = d / "layout.cpp"
    src.write_text(SRC)
    so = d / "liblayout.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    for n in ("size_generic", "size_unit", "size_frag64", "size_wrec"):
        getattr(lib, n).restype = C.c_longlong
    lib.value16.argtypes = [C.c_float, C.c_int, C.c_int]
    lib.value16.restype = C.c_uint
    return lib


def mapped(fn, n, *args):
    out = np.zeros((n, 4), np.int32)
    fn(C.c_longlong(n), *args, out.ctypes.data_as(C.POINTER(C.c_int)))
    return out


def check_cover(m, nf, KK, parts=1):
    """every (filter < nf, tap, channel[, part]) is the source of exactly one destination; the rest is padding (-1)"""
    real = m[m[:, 0] >= 0]
    assert real[:, 0].max() == nf - 1 and real[:, 1].max() == KK - 1 and real[:, 2].max() == 31 and real.min() >= 0
    key = ((real[:, 0].astype(np.int64) * KK + real[:, 1]) * 32 + real[:, 2]) * parts + real[:, 3]
    assert len(key) == nf * KK * 32 * parts and len(np.unique(key)) == len(key)
    assert np.all(m[m[:, 0] < 0][:, 0] == -1)


def pack(m, bank):
    """the table packed through the mapping: bank[f][tap * 32 + channel] at every real destination, 0 in the padding"""
    out = np.zeros(len(m), bank.dtype)
    real = m[:, 0] >= 0
    out[real] = bank[m[real, 0], m[real, 1] * 32 + m[real, 2]]
    return out


@pytest.mark.parametrize("K,nf", [(5, 156), (5, 6), (9, 4), (12, 3), (8, 2), (3, 10), (1, 17)])
def test_generic_and_group_banks(lay, K, nf):
    KK, Fpad = K * K, (nf + 7) // 8 * 8
    assert lay.weight_place(3, 7) == 3 * 32 + 7
    n = lay.size_generic(KK, Fpad)
    assert n == 32 * KK * Fpad
    bank = np.random.default_rng(K * 100 + nf).normal(size=(nf, KK * 32))
    g = mapped(lay.map_generic, n, KK, Fpad, nf)
    check_cover(g, nf, KK)
    want = np.zeros((32, KK, Fpad))                              # [channel][tap][Fpad]
    want[:, :, :nf] = bank.reshape(nf, KK, 32).transpose(2, 1, 0)
    assert pack(g, bank).tobytes() == want.tobytes()
    q = mapped(lay.map_group, n, KK, nf)
    check_cover(q, nf, KK)
    padded = np.zeros((Fpad, KK, 32))
    padded[:nf] = bank.reshape(nf, KK, 32)
    want = padded.reshape(Fpad // 8, 8, KK, 32).transpose(0, 3, 2, 1)   # [group][channel][tap][8]
    assert pack(q, bank).tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.mark.parametrize("f0,ql,nf", [(0, 8, 156), (48, 6, 156), (150, 6, 156), (4, 2, 5), (0, 4, 3)])
def test_units(lay, f0, ql, nf):
    KK = 25
    n = lay.size_unit(KK, ql)
    assert n == 32 * KK * ql
    m = mapped(lay.map_unit, n, KK, f0, ql, nf)
    bank = np.random.default_rng(f0 + ql).normal(size=(nf, KK * 32)).astype(np.float32)
    real = m[m[:, 0] >= 0]
    assert set(np.unique(real[:, 0])) == set(range(f0, min(f0 + ql, nf)))
    want = np.zeros((32, KK, ql), np.float32)                    # [channel][tap][ql]
    for q in range(ql):
        if f0 + q < nf:
            want[:, :, q] = bank[f0 + q].reshape(KK, 32).T
    assert pack(m, bank).tobytes() == want.tobytes()
    assert np.count_nonzero(m[:, 0] < 0) == 32 * KK * max(0, f0 + ql - nf)


def test_c31_border_cases(lay):
    for cs in range(81):
        right, left, bot, top = cs % 3, cs // 3 % 3, cs // 9 % 3, cs // 27
        for i in range(5):
            for j in range(5):
                assert lay.tap_outside(cs, i, j) == int(i < top or i > 4 - bot or j < left or j > 4 - right)


@pytest.mark.parametrize("K,QN,nf", [(5, 8, 156), (5, 8, 16), (9, 2, 4), (8, 4, 70), (12, 1, 33), (3, 8, 129)])
def test_f64_fragments(lay, K, QN, nf):
    """[pass][channel block][tap][q-pair][M-tile of the pass][q of the pair][lane]: lane l of M-tile m holds filter
    m * 16 + (l & 15), channel cb * 4 QN + (l >> 4) * QN + qp * QS + e"""
    KK, mtiles = K * K, (nf + 15) // 16
    passes = (mtiles + 3) // 4
    n = lay.size_frag64(KK, mtiles)
    assert n == mtiles * 8 * KK * 64
    m = mapped(lay.map_frag64, n, KK, QN, mtiles, passes, nf)
    check_cover(m, nf, KK)
    bank = np.random.default_rng(K + nf).normal(size=(nf, KK * 32))
    QS = min(QN, 2)
    QP, CB = QN // QS, 4 * QN
    want = []
    for ps in range(passes):
        m0, m1 = lay.pass_begin(ps, mtiles, passes), lay.pass_begin(ps + 1, mtiles, passes)
        assert (m0, m1) == (ps * mtiles // passes, (ps + 1) * mtiles // passes)
        for cb in range(32 // CB):
            for t in range(KK):
                for qp in range(QP):
                    for mt in range(m0, m1):
                        for e in range(QS):
                            for l in range(64):
                                fl, c = mt * 16 + (l & 15), cb * CB + (l >> 4) * QN + qp * QS + e
                                want.append(bank[fl, t * 32 + c] if fl < nf else 0.0)
    assert pack(m, bank).tobytes() == np.array(want).tobytes()


def bf16(v):
    u = np.float32(v).view(np.uint32).astype(np.uint64)
    return int(((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff)


@pytest.mark.parametrize("NV,nf", [(2, 156), (1, 156), (2, 161), (1, 7)])
def test_matrix_core_records(lay, NV, nf):
    """[pass of 160][tap][k-step][M-tile of 32][hi | lo][lane][8]: lane holds filter lane & 31 of the M-tile, channels
    kh * 16 + (lane >> 5) * 8 + j; bf16 hi / lo = round-to-nearest-even of v and of v - hi; fp16: one rounding"""
    KK = 25
    passes = (nf + 159) // 160
    n = lay.size_wrec(KK, NV, nf)
    assert n == passes * KK * 2 * 5 * NV * 64 * 8
    m = mapped(lay.map_wrec, n, KK, NV, nf)
    check_cover(m, nf, KK, parts=NV)
    want = np.full((passes, KK, 2, 5, NV, 64, 8, 4), -1, np.int32)
    for ps in range(passes):
        for mt in range(5):
            for lane in range(64):
                f = ps * 160 + mt * 32 + (lane & 31)
                if f >= nf:
                    continue
                for kh in range(2):
                    for j in range(8):
                        for v in range(NV):
                            want[ps, :, kh, mt, v, lane, j, 0] = f
                            want[ps, :, kh, mt, v, lane, j, 1] = np.arange(KK)
                            want[ps, :, kh, mt, v, lane, j, 2] = kh * 16 + (lane >> 5) * 8 + j
                            want[ps, :, kh, mt, v, lane, j, 3] = v
    got = m.copy()
    got[got[:, 0] < 0] = -1
    assert np.array_equal(got, want.reshape(-1, 4))
    rng = np.random.default_rng(8)
    vals = np.concatenate([rng.normal(0, 0.05, 200), [0.0, -0.0, 1e-8, -3e-6, 6.1e-5, 5.96e-8, 2.98e-8, 65504.0, 65519.9, 65520.0, 1e6,
                                                      -7e4, 1.0, 1.0009765625, 1.00048828125, 1.00146484375]]).astype(np.float32)
    with np.errstate(over="ignore"):
        for v in vals:
            fv = float(v)
            assert lay.value16(fv, 1, 0) == int(np.float32(v).astype(np.float16).view(np.uint16))
            hi = bf16(v)
            assert lay.value16(fv, 0, 0) == hi
            back = np.array([hi << 16], np.uint32).view(np.float32)[0]
            assert lay.value16(fv, 0, 1) == bf16(np.float32(v) - back)


@pytest.mark.parametrize("std", ["c++11", "c++17"])
def test_host_update_members_compile(tmp_path, std):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
template <typename T>
void use(pbdhost::PartsBasedDetector<T> &d, pbdhost::QP &q)
{
    std::vector<T> w = d.modelVector();
    d.setModelVector(w);
    d.setThreshold(0.5f);
    q.apply(d.handle());
}
template void use<float>(pbdhost::PartsBasedDetector<float> &, pbdhost::QP &);
template void use<double>(pbdhost::PartsBasedDetector<double> &, pbdhost::QP &);
''')
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
