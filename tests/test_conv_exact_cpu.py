"""The CPU link of the exact convolution's pinning suite (the GPU link: tests/test_gpu_conv_exact.py; the inputs:
tests/conv_exact_cases.py).  No GPU.

1. oracle.conv equals, bit for bit, a plain numpy statement of the reference's arithmetic in the response type itself
   (conv_exact_cases.plain_conv) -- on every bank the GPU tests use, at a reduced level list, and on the zero, negative-zero,
   subnormal and channel-31 cases.  oracle.conv is held to scipy within 1e-5 elsewhere; this pins its ORDER of roundings.
2. The inputs discriminate: the share of responses whose bits change when the statement fuses the multiply-add, takes the taps
   column-major, the channels in reverse, or accumulates straight into the response; and the share of channel-31 table sums
   that change when summed sorted, reversed or column-major.  The floors asserted are half the measured shares (DESIGN.md,
   "Parity bars in the tests"), rounded down to a round figure.
3. Which kernel variants the GPU tests' inputs reach, from host logic alone: strip-sequence tiles (pbd_debug_seg_tiles), the
   unit sizes of k_conv3 (conv_units restated), the channel blocks of k_conv_generic (launch_conv_stage's rule restated, the
   constants read from csrc/pbd_internal.h), the unit / group split, and the channel-31 cases of the fused path."""
import numpy as np
import pytest

import conv_exact_cases as X

DTYPES = ["float32", "float64"]


def _banks(dtn):
    """(name, group, sizes) of every bank the GPU tests use for this type"""
    out = []
    if dtn == "float32":
        out += [("5x5 x %d" % n, "conv3", (5,) * n) for n in X.CONV3_BANKS]
    out += [("mixed", "conv3", X.mixed_sizes())]
    out += [("K=%d x %d" % (K, n), "generic", (K,) * n) for K, n in (X.GENERIC_BANKS if dtn == "float32" else X.GENERIC_BANKS_F64)]
    return out


def _levels(group, dtn):
    return X.level_features("reduced_conv3" if group == "conv3" else "reduced_generic", dtn)


# ---- 1. oracle == plain statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", DTYPES)
def test_oracle_equals_the_plain_statement_on_every_bank(oracle, dtn):
    for name, group, sizes in _banks(dtn):
        filters = X.bank(sizes, dtn)
        for f in _levels(group, dtn):
            want = X.oracle_responses(oracle, f, filters)
            got = X.plain_responses(f, filters)
            assert want.dtype == got.dtype == np.dtype(dtn)
            assert np.array_equal(X.bits(want), X.bits(got)), (dtn, name, f.shape)


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("k", [5, 3])
def test_oracle_equals_the_plain_statement_on_zero_and_subnormal_cases(oracle, dtn, k):
    dt = np.dtype(dtn)
    feats, filters = X.zero_case(k, dtn)
    assert all(np.signbit(w).all() for w in filters)
    for f in feats:
        want = X.oracle_responses(oracle, f, filters)
        assert np.array_equal(X.bits(want), X.bits(X.plain_responses(f, filters)))
        if not f.any():
            assert not X.bits(want).any(), "an all-zero level under negative weights: every response is +0 by its bits"
    feats, filters = X.subnormal_case(k, dtn)
    tiny = np.finfo(dt).tiny
    nonzero = 0
    for f in feats:
        want = X.oracle_responses(oracle, f, filters)
        assert np.array_equal(X.bits(want), X.bits(X.plain_responses(f, filters)))
        assert (np.abs(want) < tiny).all(), "every response is subnormal (or zero)"
        nonzero += int(np.count_nonzero(want))
        total = want.size
    assert nonzero >= total // 2, "the oracle keeps subnormals: most responses are non-zero"


def test_oracle_equals_the_plain_statement_on_the_fused_model(oracle):
    """the edited model's filters (channel-31 weights of mixed magnitude) on real pyramid levels, including the smallest"""
    flat = X.fused_model().flatten()
    import conv_reference as R
    for dtn in DTYPES:
        filters = R.model_filters(flat, np.dtype(dtn))
        feats, _ = oracle.features_pyramid(flat, X.fused_frame(5, X.FUSED_SHAPES[0]), dtype=np.dtype(dtn).type)
        for f in feats[-2:]:
            f = np.ascontiguousarray(f)
            want = oracle.responses(flat, f)
            assert np.array_equal(X.bits(want), X.bits(X.plain_responses(f, filters))), (dtn, f.shape)


# ---- 2. the inputs discriminate ---------------------------------------------------------------------------------------------
# measured shares (this test prints them; DESIGN.md records them) and the floors under them
FLOORS = {
    ("float32", "conv3"): {"fma": 0.25, "colmajor": 0.3, "revchan": 0.4, "direct": 0.4},      # measured 0.500 0.672 0.803 0.879
    ("float32", "generic"): {"fma": 0.15, "colmajor": 0.3, "revchan": 0.35, "direct": 0.4},   # measured 0.371 0.644 0.779 0.826
    ("float64", "conv3"): {"colmajor": 0.25, "revchan": 0.35, "direct": 0.4},                 # measured 0.538 0.781 0.874
    ("float64", "generic"): {"colmajor": 0.3, "revchan": 0.35, "direct": 0.4},                # measured 0.656 0.788 0.848
}
C31_FLOORS = {"sorted": 0.35, "reversed": 0.35, "colmajor": 0.3}                              # measured 0.753 0.747 0.615


@pytest.mark.parametrize("dtn", DTYPES)
def test_another_order_or_a_fused_operation_changes_most_responses(oracle, dtn):
    """K = 1 banks are left out (one tap: only the channel order exists); for K >= 16 two filters of the bank stand for it (the
    numpy statement costs K K 32 array operations per variant).  FMA is emulated for float32 only (through float64)."""
    changed, count = {}, {}
    for name, group, sizes in _banks(dtn):
        if sizes[0] == 1:
            continue
        filters = X.bank(sizes, dtn)
        if sizes[0] >= 16:
            filters = filters[:2]
        for f in _levels(group, dtn):
            want = X.plain_responses(f, filters)
            for v in FLOORS[(dtn, group)]:
                m = X.plain_responses(f, filters, v)
                changed[(group, v)] = changed.get((group, v), 0) + int(np.sum(X.bits(m) != X.bits(want)))
                count[(group, v)] = count.get((group, v), 0) + want.size
    for (group, v), n in sorted(changed.items()):
        share = n / count[(group, v)]
        print(f"[discrimination {dtn} {group}] {v}: {share:.3f} of {count[(group, v)]} responses change")
        assert share >= FLOORS[(dtn, group)][v], (dtn, group, v, share)


def test_another_order_changes_most_channel31_table_sums():
    flat = X.fused_model().flatten()
    changed = dict.fromkeys(C31_FLOORS, 0)
    n = 0
    for f in range(flat.nfilters):
        o = int(flat.filter_offset[f])
        w25 = flat.filters_f32[o:o + 25 * X.FLEN].reshape(25, X.FLEN)[:, X.FLEN - 1]
        assert np.count_nonzero(w25 == 0) == 2 and np.count_nonzero(np.signbit(w25) & (w25 == 0)) == 1
        for cs in range(1, 81):
            want = X.bits(np.array([X.c31_sum(w25, cs)]))[0]
            n += 1
            for order in changed:
                changed[order] += int(X.bits(np.array([X.c31_sum(w25, cs, order)]))[0] != want)
    for order, c in changed.items():
        print(f"[discrimination channel-31 table] {order}: {c / n:.3f} of {n} sums change")
        assert c / n >= C31_FLOORS[order], (order, c / n)


# ---- 3. reach ---------------------------------------------------------------------------------------------------------------
def test_strip_sequence_tiles_reached(oracle):
    """the tiles of every level list and batch size the GPU tests launch k_conv3 on.

    A tile with an interior and a border segment together cannot exist: a segment that does not touch its strip's first two
    columns continues a strip from the tile before, so it is the tile's first; one that does not touch the last two is the
    tile's last; an interior segment is both, hence alone (asserted).  What the epilogue does meet is a border tile holding
    windows inside the map (cs == 0) beside windows that leave it; that is counted instead."""
    lists = {"conv3 pdf": (X.CONV3_LEVELS, 1), "large pdf": (X.LARGE_LEVELS, 1),
             "batch of 3": (X.plan_dims(oracle, X.BATCH_SHAPE), 3),
             "mixed call": ([(h, w) for _, h, w in X.mixed_plan_dims(X.MIXED_SHAPES)], 1)}
    for s in X.FUSED_SHAPES:
        lists["fused %dx%d" % s] = (X.plan_dims(oracle, s), 1)
    got = {name: X.seg_tile_counts(d, nb) for name, (d, nb) in lists.items()}
    for name, c in got.items():
        print(f"[seg tiles {name}] {c}")
        assert c["interior_and_border"] == 0
    pdf = got["conv3 pdf"]
    assert pdf["seg1"] >= 1 and pdf["seg2"] >= 1 and pdf["seg3"] >= 1 and pdf["two_levels"] >= 1 and pdf["three_levels"] >= 1
    assert got["batch of 3"]["two_frames"] >= 1 and got["batch of 3"]["two_levels"] >= 1
    frames = [f for f, _, _ in X.mixed_plan_dims(X.MIXED_SHAPES)]
    assert sorted(set(frames)) == [0, 1, 2]
    mixed_tiles = X.seg_tiles(lists["mixed call"][0], 1)
    assert any(len({frames[int(r[5 + 4 * k])] for k in range(int(r[0]))}) >= 2 for r in mixed_tiles), "a tile over two frames of the virtual frame"
    fused = [got["fused %dx%d" % s] for s in X.FUSED_SHAPES]
    assert sum(c["interior"] for c in fused) >= 1
    assert sum(c["border_tiles_with_inside_windows"] for c in fused) >= 1
    assert sum(c["two_levels"] for c in fused) >= 1 and all(sum(c["seg%d" % n] for c in fused) >= 1 for n in (1, 2, 3))


def test_unit_sizes_reached():
    c = X.internal_constants()
    units = {n: X.conv_units(n, c["NW"]) for n in X.CONV3_BANKS}
    print(f"[k_conv3 units] {units}")
    for n, u in units.items():
        assert sum(u) in (n, n + 1) and all(q in (8, 6, 4, 2) for q in u)
    assert {q for u in units.values() for q in u} == {8, 6, 4, 2}
    # a partial unit (f0 + QL > nf) of every size that can end a bank, and a bank of whole units
    partial = {u[-1] for n, u in units.items() if n % 2}
    assert partial >= {2, 4, 6} and any(n % 2 == 0 for n in units)
    assert X.conv_units(156, c["NW"]).count(8) == 9 and X.conv_units(156, c["NW"]).count(6) == 14     # the person model
    # the 5 x 5 class of the mixed bank: an odd count, ids that are not 0..nf-1 (fmap store)
    ids = [i for i, k in enumerate(X.mixed_sizes()) if k == 5]
    assert len(ids) % 2 == 1 and ids != list(range(len(ids)))
    assert len(X.fused_model().filtersw) % 2 == 1


def test_channel_blocks_reached():
    c = X.internal_constants()
    assert c["MaxK"] == 31
    hand = {4: {32: [1], 16: range(2, 8), 8: range(8, 17), 4: range(17, 31), 2: [31]},
            8: {16: [1], 8: range(2, 8), 4: range(8, 17), 2: range(17, 31), 1: [31]}}
    for itemsize, banks in ((4, X.GENERIC_BANKS), (8, X.GENERIC_BANKS_F64)):
        rule = {K: X.cblock(K, itemsize, c) for K in range(1, c["MaxK"] + 1)}
        for cb, ks in hand[itemsize].items():                       # the hand list is only a cross-check of the rule
            assert all(rule[K] == cb for K in ks), (itemsize, cb)
        used = sorted({K for K, _ in banks})
        print(f"[cblock itemsize {itemsize}] " + ", ".join(f"K={K}: {rule[K]}" for K in used))
        assert {rule[K] for K in used} == set(rule.values())
        for cb in set(rule.values()):                               # both edges of every bucket
            ks = [K for K in rule if rule[K] == cb and K != 5]
            assert min(ks) in used and max(ks) in used, (itemsize, cb)
    assert {n for _, n in X.GENERIC_BANKS} == {1, 8, 9, 17} and any(K % 2 == 0 for K, _ in X.GENERIC_BANKS)
    assert (5, 9) in X.GENERIC_BANKS_F64                            # k_conv_generic<double, false, 5>


def test_unit_and_group_split_reached():
    c = X.internal_constants()
    assert X.generic_tiles(X.LARGE_LEVELS, c) >= 1024
    assert X.split(len(X.conv_units(X.LARGE_BANK_CONV3, c["NW"])), X.generic_tiles(X.LARGE_LEVELS, c)) == len(X.conv_units(X.LARGE_BANK_CONV3, c["NW"])) > 1
    ngroups = -(-X.LARGE_BANK_GENERIC[1] // c["Q"])
    assert X.split(ngroups, X.generic_tiles(X.LARGE_LEVELS, c)) == ngroups > 1
    assert X.LARGE_BANK_CONV3 <= 17 and X.LARGE_BANK_GENERIC[1] <= 17
    # the small lists: one unit / one filter group per workgroup row, so blockIdx.y > 0 occurs
    for dims in (X.CONV3_LEVELS, X.GENERIC_LEVELS):
        wgs = X.generic_tiles(dims, c)
        assert wgs < 1024 and X.split(7, wgs) == 1 and X.split(3, wgs) == 1
    print(f"[split] large cover {X.generic_tiles(X.LARGE_LEVELS, c)} workgroups, conv3 list {X.generic_tiles(X.CONV3_LEVELS, c)}, "
          f"generic list {X.generic_tiles(X.GENERIC_LEVELS, c)}")


def test_generic_levels_hold_the_tile_edges():
    c = X.internal_constants()
    sides = {s for d in X.GENERIC_LEVELS for s in d}
    assert sides >= {1, 7, 8, 9, 31, 32, 33}
    assert any(h > c["TH"] for h, w in X.GENERIC_LEVELS) and any(w > c["TW"] for h, w in X.GENERIC_LEVELS)
    assert (1, 2) in X.GENERIC_LEVELS                               # smaller than every filter with K >= 3, in both directions
    hs = {h % 4 for h, w in X.CONV3_LEVELS if h * w}
    assert hs == {0, 1, 2, 3} and {w for h, w in X.CONV3_LEVELS} >= {1, 2, 63, 64, 65, 130}
    assert (3, 2) in X.CONV3_LEVELS and (1, 1) in X.CONV3_LEVELS
    i = X.CONV3_LEVELS.index((0, 5))
    assert 0 < i < len(X.CONV3_LEVELS) - 1


def test_channel31_cases_reached(oracle):
    """The cases of the fused path's frames equal the cases any accepted pyramid can reach.  The smallest map side the library
    accepts is found by enumerating frames upward from the smallest that pyramid_plan takes; every map side from there on is
    possible, and sides past 5 add no case (top and bottom, or left and right, are then never outside together)."""
    sbin, interval = 4, X.FUSED_INTERVAL
    smallest = None
    for side in range(1, 64):
        try:
            dims = X.plan_dims(oracle, (side, side), sbin, interval)
        except ValueError:
            continue
        smallest = min(min(d) for d in dims)
        break
    assert smallest == 3, smallest
    for side in range(side, side + 40):                  # no accepted frame gives a smaller map
        for other in (side, 3 * side):
            assert min(min(d) for d in X.plan_dims(oracle, (side, other), sbin, interval)) >= smallest
    possible = X.c31_cases_of([(h, w) for h in range(smallest, 9) for w in range(smallest, 9)])
    assert possible == X.c31_cases_of([(h, w) for h in range(smallest, 14) for w in range(smallest, 14)])
    reached = X.c31_cases_of([d for s in X.FUSED_SHAPES for d in X.plan_dims(oracle, s, sbin, interval)])
    print(f"[channel-31 cases] {len(reached)} reached of {len(possible)} reachable, of 81 table entries")
    assert reached == possible and len(possible) == 36
    # the restated tap rule agrees with the table's definition: case cs has (top + bot) rows and (left + right) columns outside
    for cs in range(81):
        right, left, bot, top = cs % 3, cs // 3 % 3, cs // 9 % 3, cs // 27
        n = sum(X.c31_outside(cs, i, j) for i in range(5) for j in range(5))
        assert n == 25 - (5 - min(top + bot, 5)) * (5 - min(left + right, 5))
