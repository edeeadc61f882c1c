"""The references of tests/test_gpu_dp_select.py, checked on the CPU: the oracle's dynamic program against a float64 brute force
over the tree on every model of the GPU table (bit for bit: the inputs of tests/dp_hard_models.py keep every sum exact), the
numpy find + walk against the oracle's argmin, and counts of what those inputs reach -- exact ties between mixtures won by the
first and by a later one, one-mixture children under parents with more, root ties, root scores equal to the threshold,
rectangle corners on exact halves -- without which the GPU comparisons could not tell `>` from `>=` or cvRound from floor(x + 0.5)."""
import numpy as np
import pytest

import dp_hard_models as D

REALS = {"f32": np.float32, "f64": np.float64}


def _slots(flat, c):
    p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
    for gp in range(p0 + 1, p1):
        par = p0 + int(flat.parentid[gp])
        for m in range(int(flat.mix_offset[par + 1] - flat.mix_offset[par])):
            yield int(flat.ptr_slot[gp]) + m


@pytest.mark.parametrize("K", D.TABLE_K)
def test_oracle_equals_brute_force_and_inputs_reach_the_ties(oracle, K):
    """rootv (bits), rooti and Ik of the oracle equal the brute force's first-wins max-sum on every level of both level sets (the
    largest, 258 cells, is still small enough to try every source cell for every cell), in float and in double.  Per level set the
    inputs hold at least 100 (cell, parent mixture) pairs whose maximum two child mixtures share with the first winning, 100 with
    a later one winning (from three mixtures on: with two, the winner of a tie is mixture 0), 1000 of a one-mixture child under a
    parent with more, and 3 root cells whose maximum two root mixtures share (K >= 2).  Counted for table2 .. table16 on the u8
    set: tie_first 1113..499, tie_later 294..1521, k1_under_many 1848..9856, root_tie 10..482."""
    model = D.table_model(K)
    flat = model.flatten()
    for set_name, dims in D.SETS.items():
        total = {}
        for rname, R in REALS.items():
            scores = D.quantised_scores(model, dims, 1000 + K, R)
            for l, s in enumerate(scores):
                for c in range(flat.ncomponents):
                    _, _, oIk, orv, ori = oracle.dp_min(flat, c, s)
                    rv, ri, Ik, reach = D.brute_force(flat, c, s)
                    where = (set_name, rname, l, dims[l], c)
                    assert np.array_equal(rv.astype(R).view(np.uint8), orv.view(np.uint8)), where
                    assert np.array_equal(ri, ori), where
                    for sl in _slots(flat, c):
                        assert np.array_equal(Ik[sl], oIk[sl]), where + (sl,)
                    if R is np.float32:
                        for k, v in reach.items():
                            total[k] = total.get(k, 0) + v
        print(f"table{K} {set_name}: {total}")
        if K >= 2:
            assert total["tie_first"] >= 100, (set_name, total)
            assert total["k1_under_many"] >= 1000, (set_name, total)
            assert total["root_tie"] >= 3, (set_name, total)
        if K >= 3:
            assert total["tie_later"] >= 100, (set_name, total)
        if K >= 5:
            assert total["root_tie_later"] >= 1, (set_name, total)


@pytest.mark.parametrize("K", [1, 2, 9])
def test_root_only_models_tie(oracle, K):
    """a root without children: rootv = max over its mixtures of response + bias, first maximum; two mixtures tie in some cells"""
    model = D.root_only_model(K)
    flat = model.flatten()
    ties = 0
    for dims in D.SETS.values():
        for s in D.quantised_scores(model, dims, 50 + K):
            _, _, _, orv, ori = oracle.dp_min(flat, 0, s)
            rv, ri, _, reach = D.brute_force(flat, 0, s)
            assert np.array_equal(rv.astype(np.float32).view(np.uint32), orv.view(np.uint32)) and np.array_equal(ri, ori)
            ties += reach["root_tie"]
    assert ties >= 100 or K == 1, ties


def _argmin_case(oracle, model, dims, seed, R, thresh):
    """find_walk against oracle.dp_argmin on every (level, component); returns the counts of threshold and half hits"""
    flat = model.flatten()
    scales = D.half_scales(len(dims))
    out = {"equal": 0, "above": 0, "below": 0, "even": 0, "odd": 0, "minus_half": 0}
    for l, s in enumerate(D.quantised_scores(model, dims, seed, R)):
        for c in range(flat.ncomponents):
            oIx, oIy, oIk, orv, ori = oracle.dp_min(flat, c, s)
            want = oracle.dp_argmin(flat, c, l, float(scales[l]), oIx, oIy, oIk, orv, ori, capacity=orv.size + 1)
            roots, sc, rects, halves = D.find_walk(flat, c, scales[l], oIx, oIy, oIk, orv, ori, thresh, R)
            assert D.same_candidates(roots, sc, rects, want), (model.name, l, c)
            t = R(np.float32(thresh))
            out["equal"] += int((orv == t).sum()); out["above"] += int((orv > t).sum()); out["below"] += int((orv < t).sum())
            for k, v in halves.items():
                out[k] += v
    return out


@pytest.mark.parametrize("rname", list(REALS))
@pytest.mark.parametrize("set_name", list(D.SETS))
def test_find_walk_reference_on_the_ragged_model(oracle, set_name, rname):
    """The numpy find + walk equals the oracle's argmin under the half-integer scales, and the inputs hold root scores equal to
    the threshold (absent from both lists: the test is a strict `>`), above and below it, and rectangle corners (x - 1) * scale
    on exact halves below even floors, below odd floors and at -0.5 (x == 0 under scale 0.5: cvRound gives -0, floor(x + 0.5)
    gives 0 as well but 0.5 -> 0 against 1, 1.5 -> 2 both, 2.5 -> 2 against 3).  Counted on the u8 set: 10 scores equal to the
    threshold; on the i16 set: 7."""
    out = _argmin_case(oracle, D.ragged_model(), D.SETS[set_name], D.RAGGED_SEED, REALS[rname], D.RAGGED_THRESH)
    print(f"ragged {set_name} {rname}: {out}")
    assert out["equal"] >= 5 and out["above"] >= 300 and out["below"] >= 300, out
    assert out["even"] >= 100 and out["odd"] >= 100 and out["minus_half"] >= 10, out


@pytest.mark.parametrize("which", ["chain", "tree"])
def test_find_walk_reference_on_160_parts(oracle, which):
    model = (D.chain_model if which == "chain" else D.tree_model)(160)
    out = _argmin_case(oracle, model, D.WALK_SETS["u8"], 160, np.float32, model.thresh)
    assert out["equal"] == 0 and out["below"] == 0 and out["above"] == sum(h * w for h, w in D.WALK_SETS["u8"]), out
    assert out["even"] >= 100 and out["odd"] >= 100 and out["minus_half"] >= 10, out


def test_the_models_validate():
    for K in D.TABLE_K:
        m = D.table_model(K)
        m.validate()
        assert max(len(f) for c in m.filterid for f in c) == K
        assert np.all(np.abs(m.biasw) <= 2.0) and np.array_equal(np.asarray(m.biasw) * 16, np.rint(np.asarray(m.biasw) * 16))
        signs = np.signbit(np.asarray(m.biasw)[np.asarray(m.biasw) == 0.0])
        assert K == 1 or (signs.any() and not signs.all()), K       # both signs of zero
    for case in range(3):
        D.shared_model(case).validate()
    for n in (160, 161):
        D.chain_model(n).validate(); D.tree_model(n).validate()
    assert np.array_equal(np.asarray(D.ragged_model(3).biasw), np.asarray(D.ragged_model(5).biasw))
