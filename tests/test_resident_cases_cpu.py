"""The inputs of the resident-result tests can catch what they are for (resident_cases.py; no GPU here): the table is total and
every cell quotes include/pbd.h verbatim; any two scenes differ at every address they share and in every list; scenes of different
geometry differ in a level's shape and in an address only the earlier one has; the step sequences are deterministic and cover
every transition between the writers' effects."""
import os

import numpy as np
import pytest

import resident_cases as RC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pbd.h")
SCENES = tuple(RC.SCENE_FRAMES)
PAIRS = [(a, b) for a in SCENES for b in SCENES if a != b]
STAGES = tuple(k for k, _ in RC.STAGES)


def test_the_table_is_total_and_quotes_the_header():
    lines = open(HEADER).read().split("\n")
    kinds = {RC.VALUE, RC.STATE, RC.INVALID, RC.UNSUPPORTED, RC.PREV, RC.PREV_PLAIN}
    assert len(RC.WRITERS) == len(RC.WRITER) >= 40 and len(set(RC.READERS)) == len(RC.READERS) == 13
    assert len(RC.TABLE) == len(RC.WRITERS) * len(RC.READERS)
    for w in RC.WRITERS:
        for r in RC.READERS:
            cell = RC.TABLE[(w.name, r)]
            assert cell.kind in kinds, (w.name, r)
            assert cell.quote and len(cell.quote) >= 30 and any(cell.quote in line for line in lines), (w.name, r, cell.quote)
    assert any(RC.Q_FLIGHT in line for line in lines) and "PBD_ERR_STATE" in lines[[RC.Q_FLIGHT in l for l in lines].index(True) + 1]
    # a transparent or refused writer decides nothing itself; a writer that leaves a whole result decides every cell
    for w in RC.WRITERS:
        kinds_of = {RC.TABLE[(w.name, r)].kind for r in RC.READERS}
        if w.row in ("same", "refused"):
            assert kinds_of == {RC.PREV}, w.name
        elif w.scene:
            assert not kinds_of & {RC.PREV, RC.PREV_PLAIN}, w.name
    # the writers the issue names, the calls include/pbd.h says leave the result alone, a refused call of each writing family
    for name in ("detect", "detect_batch", "detect_batch_device_out", "submit_wait", "detect_frames", "detect_frames_device_out",
                 "detect_latent", "features_pyramid", "conv_pdf", "dp_min", "conv_set_filters", "set_model_vector", "set_thresh",
                 "warp_positives", "set_level_shard", "max_marginals", "suppress", "candidate_mask", "part_poses", "boxes3d",
                 "cluster_parts", "augment_frames", "top_k", "grid_nms", "depth_prune"):
        assert name in RC.WRITER, name
    assert {w.scene for w in RC.WRITERS if w.scene} == set(SCENES)
    assert sum(w.row == "refused" for w in RC.WRITERS) == len(RC.REFUSED) == 14


def test_a_new_handle_and_the_stack_of_effects():
    st = RC.State()
    assert all(st.kind(r) == RC.STATE for r in RC.READERS)
    st.wrote(RC.WRITER["detect_batch"])
    assert st.scene == "b3" and st.kind("stage_rootv") == RC.VALUE and st.kind("get_marginals") == RC.STATE
    st.wrote(RC.WRITER["max_marginals"], 2)
    assert st.kind("get_marginals") == RC.VALUE and st.kind("examples") == RC.VALUE and st.mm_frame == 2
    st.wrote(RC.WRITER["refused_detect"])
    st.wrote(RC.WRITER["grid_nms"])
    assert st.stack == ["detect_batch", "max_marginals"]
    st.wrote(RC.WRITER["conv_set_filters"])
    assert [st.kind(r) for r in ("stage_features", "pyramid_image", "stage_responses", "get_marginals", "examples")] == \
        [RC.VALUE, RC.VALUE, RC.STATE, RC.STATE, RC.STATE]
    st.wrote(RC.WRITER["warp_positives"])
    assert all(st.kind(r) == RC.STATE for r in RC.READERS)
    st.wrote(RC.WRITER["detect_latent"])
    assert st.stack == ["detect_latent"] and st.kind("stage_features") == RC.VALUE and st.kind("max_marginals") == RC.STATE
    st.wrote(RC.WRITER["set_model_vector"])
    assert all(st.kind(r) == RC.STATE for r in RC.READERS)       # nothing of a latent result stays readable
    st.wrote(RC.WRITER["detect_frames"])
    assert st.kind("max_marginals") == RC.UNSUPPORTED and st.kind("dp_argmin") == RC.STATE and st.kind("argmin_device_out") == RC.VALUE


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_any_two_scenes_differ_wherever_they_can_be_confused(dtype):
    """every ordered pair, every (stage, frame, level) valid in both: the planes differ in bytes whenever their shapes agree; so do
    the level images, the record lists and the example values.  Nothing is left out."""
    compared = 0
    for a, b in PAIRS:
        A, B = RC.scene(a, dtype), RC.scene(b, dtype)
        for f, l in A.addresses():
            if not B.valid(f, l):
                continue
            for stage in STAGES:
                pa, pb = A.plane(stage, f, l), B.plane(stage, f, l)
                if pa.shape == pb.shape:
                    compared += 1
                    assert pa.tobytes() != pb.tobytes(), (a, b, stage, f, l)
            ia, ib = A.image(f, l), B.image(f, l)
            if ia.shape == ib.shape:
                assert ia.tobytes() != ib.tobytes(), (a, b, "image", f, l)
        assert A.records().tobytes() != B.records().tobytes() and len(A.records()) != len(B.records()), (a, b)
        assert A.sel().tobytes() != B.sel().tobytes(), (a, b)
        assert A.examples()[1].tobytes() != B.examples()[1].tobytes(), (a, b)
        assert A.part_scores()[2].tobytes() != B.part_scores()[2].tobytes(), (a, b)
    # a, a2 and g share 12 levels of one shape (6 ordered pairs), s and frame 0 of mix share 9 (2 ordered pairs); 4 stages each
    assert compared == (6 * 12 + 2 * 9) * 4
    # the max-marginals of two frames of a batch, and of two scenes of one size, differ plane by plane
    b3 = RC.scene("b3", dtype)
    for l in range(b3.nlevels(0)):
        for key, _ in RC.WHAT[:2]:
            assert b3.marginals(0)[l][key].tobytes() != b3.marginals(2)[l][key].tobytes(), (key, l)
            k = min(l, 11)
            assert RC.scene("a", dtype).marginals(0)[k][key].tobytes() != RC.scene("a2", dtype).marginals(0)[k][key].tobytes()


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_scenes_of_different_geometry_have_addresses_of_their_own(dtype):
    def geometry(s):
        return [[s.shape(f, l) for l in range(s.nlevels(f))] for f in range(s.nframes)]
    def lost(A, B):
        return [(f, l) for f, l in A.addresses() if not B.valid(f, l)]
    differing = 0
    for a, b in PAIRS:
        A, B = RC.scene(a, dtype), RC.scene(b, dtype)
        if geometry(A) == geometry(B):
            # the same maps from another channel count: the level images differ in size (pbd_get_pyramid_image)
            assert A.cn == B.cn or A.image(0, 0).nbytes != B.image(0, 0).nbytes, (a, b)
            continue
        differing += 1
        # a level both have whose shape differs; and, in one order of the two at least, an address only the earlier scene has
        # (s and mix: frame 0 of mix has the size of s, both sizes being given; what tells them apart is frame 1 of mix, and the
        #  bytes of every plane they share, compared above)
        if {a, b} != {"s", "mix"}:
            assert any(A.shape(f, l) != B.shape(f, l) for f, l in A.addresses() if B.valid(f, l)), (a, b)
        assert lost(A, B) or lost(B, A), (a, b)
    assert differing == 2 * (15 - 3)                   # a, a2 and g share their geometry
    for a, b in (("b3", "s"), ("a", "mix"), ("b3", "a2"), ("mix", "s"), ("a", "s")):
        assert lost(RC.scene(a, dtype), RC.scene(b, dtype)), (a, b)
    assert RC.scene("a", dtype).image(0, 0).shape[2] == 3 and RC.scene("g", dtype).image(0, 0).shape[2] == 1
    # the probed addresses go past every scene, and every buffer a reader passes holds the largest plane and image of any scene
    for n in SCENES:
        s = RC.scene(n, dtype)
        assert s.nframes < max(RC.PROBE_FRAMES) and max(s.nlevels(f) for f in range(s.nframes)) < max(RC.PROBE_LEVELS)
        assert len(s.records()) < RC.CAP <= RC.MAX_CANDIDATES
        for f, l in s.addresses():
            assert s.image(f, l).nbytes <= RC._max_bytes()[1]
            assert max(s.plane(k, f, l).nbytes for k in STAGES) <= RC._max_bytes()[0]
            assert 6 * s.shape(f, l)[0] * s.shape(f, l)[1] * 8 <= RC._max_bytes()[0]


def test_the_latent_twin_of_the_model_is_the_model():
    """every (component, part, mixture) of the tiny model has a filter of its own already, in global mixture order: the stages of
    a latent run with nothing masked are those of a detect call"""
    from partsbaseddetector_amd import examples as E
    u = E.unique_model(RC.model()).flatten()
    f = RC.flat()
    assert list(u.filterid) == list(f.filterid) == list(range(f.nfilters))
    assert u.filters_f64.tobytes() == f.filters_f64.tobytes()
    a = RC.scene("a", "float32")
    assert a.latent()[5:6].view(np.float32)[0] == max(r[5:6].view(np.float32)[0] for r in a.records())


def test_the_option_mirrors_cut_the_list_and_off_is_the_oracle():
    a = RC.scene("a", "float32")
    full = RC.emitted(a, RC.OFF)
    assert full.tobytes() == a.records().tobytes()
    depth = (525.0, 450.0, 0.35)
    for st in (RC.settings(root_nms=2), RC.settings(top_k=7), RC.settings(nms=0.3), RC.settings(dprune=depth),
               RC.settings(root_nms=2, top_k=7, nms=0.3)):
        cut = RC.emitted(a, st)
        assert 0 < len(cut) < len(full), st
        assert {r.tobytes() for r in cut} <= {r.tobytes() for r in full}
    assert len(RC.emitted(a, RC.settings(top_k=7))) == 7
    arg = RC.emitted(a, RC.settings(walk="argmax"))
    assert arg[:, :8].tobytes() == full[:, :8].tobytes() and arg.tobytes() != full.tobytes()
    assert RC.emitted(a, RC.settings(root_nms=2, walk="argmax"), False).tobytes() == arg.tobytes()      # pbd_dp_argmin: the walk only


def test_the_step_sequences_are_deterministic_and_cover_every_transition():
    circuit = RC.class_circuit()
    n = len(RC.CLASSES)
    assert len(circuit) == n * n + 1 and circuit[0] == circuit[-1]
    assert len(set(zip(circuit, circuit[1:]))) == n * n
    seen = set()
    for seed in RC.WALK_SEEDS:
        steps = RC.walk_steps(seed)
        RC.walk_steps.cache_clear()
        assert steps == RC.walk_steps(seed) and len(steps) == RC.WALK_STEPS
        assert all(s[0] in ("write", "read", "set") for s in steps)
        assert sum(s[0] == "read" for s in steps) >= 5 and sum(s[0] == "set" for s in steps) >= 2
        seen |= RC.class_transitions(steps)
    assert len(seen) == n * n == 64
    assert {RC.writer_class(w.name) for w in RC.WRITERS} == set(RC.CLASSES)
