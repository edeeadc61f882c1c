"""PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY without a GPU: the A-fragment layout's one definition (any_frag_source,
partsbaseddetector_amd/csrc/pbd_layout.h) covers every weight exactly once with padding as the only other slots, and the
one-hot inputs of the GPU test discriminate: their emulated reference is an fp32 number, and a reference that lacks either
lo term fails conv_reference.check by a wide margin at every side used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_any_cases as A
import conv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")

SRC = r'''
#include "pbd_layout.h"
using namespace pbd;
extern "C" {
void map_any(long long n, int KK, int CB, int NV, int nf, int *out)
{ for (long long i = 0; i < n; ++i) { int part = 0; WeightSrc s = any_frag_source(i, KK, CB, NV, nf, &part); out[4*i] = s.f; out[4*i+1] = s.t; out[4*i+2] = s.c; out[4*i+3] = part; } }
long long size_any(int KK, int CB, int NV, int nf) { return any_frag_size(KK, CB, NV, nf); }
int steps_any(int KK, int CB) { return any_steps(KK, CB); }
int passes_any(int mtiles) { return mfma_passes(mtiles); }
int pass_begin(int ps, int mtiles, int passes) { return mfma_pass_begin(ps, mtiles, passes); }
}
'''


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout_any")
    src = d / "layout.cpp"
    src.write_text(SRC)
    so = d / "liblayout_any.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    lib.size_any.restype = C.c_longlong
    return lib


def _map(lay, KK, CB, NV, nf):
    n = lay.size_any(KK, CB, NV, nf)
    out = np.zeros((n, 4), np.int32)
    lay.map_any(C.c_longlong(n), KK, CB, NV, nf, out.ctypes.data_as(C.POINTER(C.c_int)))
    return n, out


@pytest.mark.parametrize("NV", [2, 1])
@pytest.mark.parametrize("K", [1, 2, 5, 6, 19, 31])
def test_fragment_layout_covers_every_weight_once(lay, K, NV):
    """every (filter < nf, tap, channel, part) exactly once, everything else "pad", the size function = the entries; for
    each channel block the kernel may stage (the host picks one per side; the layout holds for all three)"""
    KK = K * K
    for nf in (1, 31, 33, 161):
        if K == 31 and nf == 161:
            cbs = [A.staging_cb(K, NV == 1)]          # (4.9 M entries per block size: the one the host picks)
        else:
            cbs = [32, 16, 8]
        for CB in cbs:
            mtiles = (nf + 31) // 32
            n, m = _map(lay, KK, CB, NV, nf)
            assert n == mtiles * (32 // CB) * lay.steps_any(KK, CB) * NV * 512
            real = m[m[:, 0] >= 0]
            assert real.min() >= 0 and real[:, 0].max() == nf - 1 and real[:, 1].max() == KK - 1 and real[:, 2].max() == 31
            assert real[:, 3].max() == NV - 1
            key = ((real[:, 0].astype(np.int64) * KK + real[:, 1]) * 32 + real[:, 2]) * NV + real[:, 3]
            assert len(key) == nf * KK * 32 * NV and len(np.unique(key)) == len(key), (K, nf, CB)
            assert np.all(m[m[:, 0] < 0][:, 0] == -1)
            # the pad slots are the filters past nf and, with two taps per step and K*K odd, the last step's second tap
            pad_taps = (32 // CB) * (2 * lay.steps_any(KK, CB) - KK) * 8 * 32 * mtiles * NV if CB == 8 else 0
            assert n - len(real) == (mtiles * 32 - nf) * KK * 32 * NV + pad_taps


@pytest.mark.parametrize("K,CB", [(3, 32), (3, 16), (3, 8), (2, 8)])
def test_fragment_layout_is_the_documented_order(lay, K, CB):
    """[pass][channel block][step][M-tile of the pass][part][lane][8] with lane (r, hh) -> filter, tap, channel as the header
    states them, restated with numpy for a class of two passes (161 filters: 3 + 3 M-tiles)"""
    KK, NV, nf = K * K, 2, 161
    mtiles, steps = 6, lay.steps_any(KK, CB)
    assert lay.passes_any(mtiles) == 2 and [lay.pass_begin(p, mtiles, 2) for p in range(3)] == [0, 3, 6]
    n, m = _map(lay, KK, CB, NV, nf)
    m = m.reshape(2, 32 // CB, steps, 3, NV, 64, 8, 4)
    ps, cb, s, mt, part, lane, j = np.meshgrid(*[np.arange(d) for d in m.shape[:-1]], indexing="ij")
    f = (ps * 3 + mt) * 32 + (lane & 31)
    hh = lane >> 5
    if CB == 32:
        t, c = s >> 1, (s & 1) * 16 + hh * 8 + j
    elif CB == 16:
        t, c = s, cb * 16 + hh * 8 + j
    else:
        t, c = 2 * s + hh, cb * 8 + j
    pad = (f >= nf) | (t >= KK)
    assert np.array_equal(m[..., 0] < 0, pad)
    keep = ~pad
    for col, want in ((0, f), (1, t), (2, c), (3, part)):
        assert np.array_equal(m[..., col][keep], want[keep]), col


def test_staging_rule_switches():
    """the sides the GPU test runs sit on both sides of every change of the host's staging rule"""
    for f16, sides in ((False, A.SIDES_BF16), (True, A.SIDES_F16)):
        cb = [A.staging_cb(k, f16) for k in range(1, 32)]
        for k in range(1, 31):
            if cb[k - 1] != cb[k]:
                assert k in sides and k + 1 in sides, (f16, k)
        assert set(cb) == {32, 16, 8} and 1 in sides and 31 in sides


ONEHOT_K = [1, 2, 3, 4, 6, 7, 12, 18, 19, 31]


@pytest.fixture(scope="module")
def level():
    return A.onehot_features(5, [(9, 37)])[0]


@pytest.mark.parametrize("k", ONEHOT_K)
def test_onehot_reference_is_fp32_and_lo_mutants_fail(level, k):
    """the emulated reference is exactly representable in fp32; a reference with either lo term dropped fails the check at
    every side (13 x the bound at k = 31 .. 416 x at k = 1); M == 0 elements are checked for exact zeros, not skipped"""
    ref, M = A.onehot_ref(level, k, "mfma")
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    n = R.products("mfma", k * k * R.FLEN)
    ok = R.check(ref.astype(np.float32), ref, M, n, R.U32)
    assert ok.ok and ok.worst == 0.0
    zero = float((M == 0).mean())
    assert (zero == 0.0) if k == 1 else (zero > 0.0)
    if k == 31:
        assert 0.7 < zero < 0.8
    assert np.all(ref[M == 0] == 0)
    for drop in (1, 2):
        mut, _ = A.onehot_ref(level, k, "mfma", drop=drop)
        s = R.check(mut.astype(np.float32), ref, M, n, R.U32)
        assert not s.elem_ok and s.worst > 10.0, (k, drop, s)
        assert np.all(mut[M == 0] == 0)
    # fp16 mode: both operands are fp16 numbers, the response is the rounded product
    r16, M16 = A.onehot_ref(level, k, "f16")
    assert np.array_equal(M16, M)
    got16 = R.f16_response(r16.astype(np.float32))
    assert R.f16_check(got16, r16, M16, k * k * R.FLEN).ok
    # and the vector modes' result (the full product, lo*lo included) is a different fp32 number wherever the feature is a
    # cell of the map (a border cell of channel 31 is 1: no lo term)
    differs = A.onehot_differs(level, k)
    _, where = A.onehot_bank(k)
    for f, (t, c, v) in enumerate(where):
        if c != 31:
            assert np.array_equal(differs[f], M[f] > 0)
    assert differs.any()


@pytest.mark.parametrize("k", ONEHOT_K)
def test_onehot_reference_is_conv_reference(level, k):
    """onehot_ref restates conv_reference.ref64 on the products that are not identically zero: equal on whole small banks
    and on a stride of the large banks' filters"""
    filters, _ = A.onehot_bank(k)
    ids = list(range(k * k)) if k <= 4 else list(range(0, k * k, max(1, k * k // 5)))
    for mode in ("mfma", "f16"):
        want, Mw = R.ref64(level, [filters[i] for i in ids], mode=mode)
        got, Mg = A.onehot_ref(level, k, mode, filters=ids)
        assert np.array_equal(got, want) and np.array_equal(Mg, Mw), (k, mode)
