"""The built cases of tests/latent_hard_cases.py, checked without a GPU: every case meets the condition it is built for, asserted
on the yardstick alone (partsbaseddetector_amd/examples.py on the oracle), so that a case cannot silently stop exercising its
edge; and the stage-by-stage yardstick of that file gives examples.latent_search's answer."""
from fractions import Fraction

import numpy as np
import pytest

import latent_hard_cases as L
from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import model as M

MASKED = np.float32(E.MASKED)


def level0(name):
    st = L.latent_yardstick(name)[0]
    return st, st["resp"][0], float(st["scales"][0])


@pytest.mark.parametrize("name", sorted(L.LATENT_CASES))
def test_stage_yardstick_is_latent_search(oracle, name):
    case = L.latent_case(name)
    for walk in (("reference", "argmax") if name in L.BOTH_WALKS else ("reference",)):
        for f, st in enumerate(L.latent_yardstick(name)):
            want = E.latent_search(case.model, case.frames[f], case.boxes[f], L.widened(case.overlap),
                                   None if case.mixtures is None else case.mixtures[f], np.float32, walk)
            assert (st["level"], st["component"], st["root_x"], st["root_y"]) == (want["level"], want["component"], want["root_x"],
                                                                                   want["root_y"])
            assert float(np.float32(st["score"])) == want["score"] and st["found"] == want["found"]
            assert st["placement"][walk] == want["placement"] and np.array_equal(st["parts"][walk], want["parts"])


def test_half_is_masked_and_one_float_below_is_kept(oracle):
    st, resp, scale = level0("half")
    assert scale == 4.0 and L.latent_case("half").overlap == np.float32(0.5) == 0.5
    at = L.positions_with_iou(resp.shape[1:], 5, scale, L.HALF_BOX, Fraction(1, 2))
    assert len(at) == 6
    for x, y in at:
        x1, y1, x2, y2 = (int(v) for v in E.part_rects(x, y, 5, scale, np.float32))
        assert (x2 - x1 + 1, y2 - y1 + 1) == (20, 20)
        assert L.HALF_BOX[0] <= x1 and x2 <= L.HALF_BOX[2] and L.HALF_BOX[1] <= y1 and y2 <= L.HALF_BOX[3]   # wholly inside
        assert L.exact_iou(x, y, 5, scale, L.HALF_BOX) == Fraction(400, 800)
        assert np.all(resp[:, y, x] == MASKED)
    below = L.latent_case("below_half")
    assert below.overlap < 0.5 and np.nextafter(below.overlap, np.float32(1)) == np.float32(0.5)
    kept = L.latent_yardstick("below_half")[0]["resp"][0]
    for x, y in at:
        assert np.all(kept[:, y, x] != MASKED)
    # nothing else differs between the two calls at this level: the six positions are where the threshold decides
    differ = np.argwhere(np.any(kept != resp, axis=0))
    assert sorted((int(x), int(y)) for y, x in differ) == sorted(at)


def test_seven_tenths_is_kept_by_the_float_and_masked_by_the_decimal(oracle):
    st, resp, scale = level0("seven_tenths")
    case = L.latent_case("seven_tenths")
    at = L.positions_with_iou(resp.shape[1:], 5, scale, L.TENTHS_BOX, Fraction(7, 10))
    assert len(at) == 1
    (x, y), = at
    assert L.exact_iou(x, y, 5, scale, L.TENTHS_BOX) == Fraction(280, 400)
    assert L.widened(case.overlap) < 0.7 and 280 / 400 == 0.7
    assert np.all(resp[:, y, x] != MASKED)                                  # the kernel's reading: float32(0.7) widened
    rect = E.part_rects(np.int64(x), np.int64(y), 5, scale, np.float32)
    assert bool(E.overlap_passes(rect, L.TENTHS_BOX, L.widened(case.overlap))) and not bool(E.overlap_passes(rect, L.TENTHS_BOX, 0.7))
    # and it decides the answer: that position is the best root
    assert (st["level"], st["root_x"], st["root_y"]) == (0, x, y)


def test_sizes_models_have_every_filter_size(oracle):
    want = {"1_3_6": [1, 3, 6, 1, 3, 6, 1, 3], "9_12_5": [9, 12, 5] * 4, "1": [1] * 8, "5": [5] * 8}
    for name, ks in want.items():
        flat = L.sizes_model(name).flatten()
        assert list(flat.filter_ksize) == ks and flat.max_parts == 4
        assert list(flat.parentid) == [-1, 0, 0, 1]                          # a grandchild: the walk reads a walked parent
    # the lane arithmetic of k_ex_gather: k * CPC chunks per window row against the 64 lanes of a wave, CPC = 8 (float), 16 (double)
    for cpc in (8, 16):
        rows = {k: k * cpc for k in (1, 3, 5, 6, 9, 12)}
        assert rows[1] < 64 and rows[3] < 64 and rows[12] > 64 and rows[9] > 64
        assert any(64 % r for r in rows.values()) and {k % 2 for k in rows} == {0, 1}
    for name in ("sizes_1_3_6", "sizes_9_12_5"):
        for dt in ("float32", "float64"):
            st = L.latent_yardstick(name, dt)[0]
            assert st["found"]
            assert len({m for (_, _, m) in st["placement"]["argmax"]}) > 1
            # every filter size of the model has a plane that keeps some position of the pyramid and masks others, so each size's
            # rectangle decides somewhere; the mixtures of a part (of different sizes) are masked differently, so a plane mapped
            # to another mixture's size would show
            T = st["resp"][0].dtype.type
            kept = [np.concatenate([(r[g] != T(E.MASKED)).ravel() for r in st["resp"]]) for g in range(len(st["resp"][0]))]
            ks = [int(k) for k in st["uflat"].filter_ksize]
            assert {k for g, k in enumerate(ks) if kept[g].any() and not kept[g].all()} == set(ks)
            for p in range(4):
                g0, g1 = int(st["uflat"].mix_offset[p]), int(st["uflat"].mix_offset[p + 1])
                for a in range(g0, g1):
                    for b in range(a + 1, g1):
                        assert ks[a] != ks[b] and not np.array_equal(kept[a], kept[b])


def test_mixtures_cases(oracle):
    case = L.latent_case("mixtures_fixed")
    assert min(case.mixtures[0]) >= 0 and sorted(set(np.sign(case.mixtures[1]))) == [-1, 0, 1]
    ys = L.latent_yardstick("mixtures_fixed")
    for f, st in enumerate(ys):
        assert st["found"]
        for p, (_, _, m) in enumerate(st["placement"]["argmax"]):
            assert case.mixtures[f][p] in (-1, m)
        for p, fixed in enumerate(case.mixtures[f]):          # over the pyramid: a fixed part keeps its mixture's plane alone
            g0 = int(st["uflat"].mix_offset[p])
            gone = [all(np.all(r[g0 + m] == MASKED) for r in st["resp"]) for m in range(3)]
            assert gone == [fixed != m for m in range(3)] if fixed >= 0 else not all(gone)
    # frame 1's fixed mixtures are not the free search's: the fix changes the answer
    free = L.latent_stages(case.model, case.frames[1], case.boxes[1], L.widened(case.overlap))
    assert any(fx >= 0 and fx != m for fx, (_, _, m) in zip(case.mixtures[1], free["placement"]["argmax"]))
    never = L.latent_case("mixtures_never")
    st = L.latent_yardstick("mixtures_never")[0]
    assert not st["found"] and never.mixtures[0][1] == 1 and int(st["uflat"].filter_ksize[3]) == 1
    for lvl, resp in enumerate(st["resp"]):
        assert np.all(resp[2] == MASKED) and np.all(resp[3] == MASKED)      # part 1: mixture 0 not allowed, mixture 1 never passes
        ys_, xs_ = np.mgrid[0:resp.shape[1], 0:resp.shape[2]]
        assert not E.overlap_passes(E.part_rects(xs_, ys_, 1, st["scales"][lvl], np.float32), never.boxes[0][1], 0.5).any()
    assert L.latent_stages(never.model, never.frames[0], never.boxes[0], 0.5)["found"]      # free, the same boxes find one


def tied_offsets(st):
    flat = np.concatenate([r.ravel() for r in st["rootv"]])
    return np.nonzero(flat == st["score"])[0]


def test_ties(oracle):
    for dt in ("float32", "float64"):
        st = L.latent_yardstick("ties", dt)[0]
        assert all(not f.any() for f in st["feats"])                       # every feature 0 ...
        assert all(np.all((r == 0) | (r == r.dtype.type(E.MASKED))) for r in st["resp"])   # ... so every kept response too
        assert (st["level"], st["component"], st["root_x"], st["root_y"]) == (0, 0, 4, 6) and st["found"]
        per_level = [(rv == st["score"]).sum(axis=(1, 2)) for rv in st["rootv"]]
        assert list(per_level[0]) == [27, 27]
        assert sum(1 for n in per_level if n.any()) == 7 and all(n[0] == n[1] for n in per_level)
        tied = tied_offsets(st)
        first = int(tied[0])
        assert first == L.root_offset(st, 0, 0, 4, 6)
        # one thread of k_latent_best meets the value again (its own scan's rule), another thread with a lower index meets it
        # only later (the tree's rule)
        assert any((t - first) % L.MASK_THREADS == 0 for t in tied[1:])
        assert any(t % L.MASK_THREADS < first % L.MASK_THREADS for t in tied[1:])
        mixed = L.latent_yardstick("ties_mixed", dt)
        assert [len(s["feats"]) for s in mixed] != [len(mixed[1]["feats"])] * 3      # pyramids of different depths
        st = mixed[1]
        tied = tied_offsets(st)
        first = int(tied[0])
        assert first == L.root_offset(st, st["level"], st["component"], st["root_x"], st["root_y"])
        assert first >= L.MASK_THREADS
        assert any(t % L.MASK_THREADS < first % L.MASK_THREADS for t in tied[1:])


def test_overlap_extremes(oracle):
    from oracle import oracle as O
    for dt in (np.float32, np.float64):
        st = L.latent_yardstick("keep_all", dt.__name__)[0]
        for lvl, feat in enumerate(st["feats"]):
            assert st["resp"][lvl].tobytes() == O.responses(st["uflat"], feat).tobytes()     # nothing masked
        assert st["found"]
        st = L.latent_yardstick("keep_none", dt.__name__)[0]
        assert all(np.all(r == dt(E.MASKED)) for r in st["resp"]) and not st["found"]
        st = L.latent_yardstick("int32_box", dt.__name__)[0]
        assert all(not np.any(r == dt(E.MASKED)) for r in st["resp"]) and st["found"]
    b = L.INT32_BOX
    assert (b[2] - b[0] + 1) * (b[3] - b[1] + 1) == 2 ** 64 and float(2 ** 64) == 2.0 ** 64
    assert L.exact_iou(0, 0, 9, 4.0, b) == Fraction(36 * 36, 2 ** 64) > 0 == L.latent_case("int32_box").overlap
    assert np.isposinf(L.latent_case("keep_none").overlap) and L.latent_case("keep_all").overlap == -1


def test_bad_records_plan(oracle):
    flat = L.bad_model().flatten()
    shapes = []
    for (rows, cols) in L.BAD_FRAMES:
        fm = E.FrameMaps(flat, np.zeros((rows, cols, 3), np.uint8))
        shapes.append(L.level_shapes(fm))
    nlevels = [len(s) for s in shapes]
    entries = L.bad_entries(nlevels, shapes, flat.ncomponents)
    reasons = [r for _, r in entries if r]
    assert reasons == ["frame below 0", "frame at nframes", "level below 0", "level at this frame's own count", "component -1",
                       "component NC", "root x -1", "root y at rows"]
    for k, ((f, c, l, x, y), reason) in enumerate(entries):
        ok = 0 <= f < 3 and 0 <= l < nlevels[f] and 0 <= c < flat.ncomponents and 0 <= x < shapes[f][l][1] and 0 <= y < shapes[f][l][0]
        assert ok == (reason is None), k
        if reason is not None:                                              # bad records sit between good ones
            assert entries[k - 1][1] is None and entries[k + 1][1] is None
    (f, c, l, x, y), = [e for e, r in entries if r == "level at this frame's own count"]
    assert f == 0 and l == nlevels[0] < nlevels[1]                       # in the virtual level table it is frame 1's level 0
    (f, c, l, x, y), = [e for e, r in entries if r == "root y at rows"]
    assert y == shapes[f][l][0] and x < shapes[f][l][1]
    assert {f for (f, *_), r in entries if r is None} == {0, 1, 2}


def test_grid_caps(oracle):
    from oracle import oracle as O
    person = M.synthetic_person_model().flatten()
    plan = O.pyramid_plan(480, 640, person.sbin, person.interval)
    cells = sum(int(r) * int(c) for r, c in L.plan_maps(plan))
    assert cells == 140725 and int(person.mix_offset[-1]) == 156
    assert cells * 156 == 21953100 > L.MASK_GRID * L.MASK_THREADS
    shapes = L.level_shapes(L.frame_maps("person", "120x160"))
    total, pos = L.seeded_positions(shapes, L.GATHER_RECORDS)
    assert total == 7431 and len(set(pos)) == L.GATHER_RECORDS == 1300
    assert L.GATHER_RECORDS * person.max_parts > L.GATHER_WAVES * L.GATHER_GRID
    assert {l for l, _, _ in pos} == set(range(len(shapes)))


def test_built_records_touch_every_border(oracle):
    for name in L.SIZES:
        fm = L.frame_maps("sizes", name)
        shapes = L.level_shapes(fm)
        entries = L.built_entries(fm.flat, shapes)
        assert len(entries) == 27 and {l for (_, _, l, _, _) in entries} == {0, len(shapes) // 2, len(shapes) - 1}
        for l in {e[2] for e in entries}:
            rows, cols = shapes[l]
            pts = {(x, y) for (_, _, ll, x, y) in entries if ll == l}
            assert {(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1), (cols // 2, rows // 2)} <= pts and len(pts) == 9
