"""The conditions the pipelined / pooled GPU tests rely on, checked on the CPU oracle's lists (tests/pipeline_cases.py)."""
import numpy as np

import pipeline_cases as PC


def test_counts_put_the_batches_on_both_sides_of_the_read_back_guess():
    assert len(PC.batch_records("large")) > PC.GUESS          # the speculative read-back's first guess is too short
    assert 0 < len(PC.batch_records("small")) < PC.GUESS
    assert len(PC.batch_records("large")) <= PC.MAX_CANDIDATES
    assert len(PC.batch_records("large")) > 100 > 8           # the capacities the failed waits use


def test_blank_frames_hold_a_handful_and_A_overflows_a_list_of_64():
    assert 0 < len(PC.frame_records("Z")) <= 8
    assert 0 < len(PC.frame_records("Z64")) <= 8
    assert len(PC.frame_records("A")) > 64
    assert len(PC.frame_records("B")) > 8                      # capacity 8 fails on A and on B, not on the blank frames


def test_every_frame_of_a_batch_has_one_shape_and_fits_the_handle():
    for name, keys in PC.BATCHES.items():
        shapes = {PC.frames()[k].shape for k in keys}
        assert len(shapes) == 1, (name, shapes)
        assert 1 <= len(keys) <= PC.MAX_BATCH
    assert PC.frames()["Z"].shape == PC.frames()["A"].shape and PC.frames()["Z64"].shape == PC.frames()["B"].shape


def test_batches_are_distinct_and_records_are_in_batch_order():
    lists = [PC.batch_records(n) for n in PC.BATCHES]
    for i, a in enumerate(lists):
        for b in lists[i + 1:]:
            assert a.shape != b.shape or not np.array_equal(a, b)      # a result handed back for the wrong batch is seen
    per_frame = [PC.frame_records(k) for k in ("A", "A2", "B", "C", "C1", "C2")]
    for i, a in enumerate(per_frame):
        for b in per_frame[i + 1:]:
            assert a.shape != b.shape or not np.array_equal(a, b)
    for name, keys in PC.BATCHES.items():
        rec = PC.batch_records(name)
        assert rec.shape[1] == PC.stride() and rec.dtype == np.int32
        k = [tuple(r[[0, 2, 1, 4, 3]]) for r in rec]
        assert k == sorted(k)
        assert set(rec[:, 0]) <= set(range(len(keys)))


def test_mirror_of_the_blank_frame_keeps_something():
    z = PC.batch_records("blank")
    kept = PC.mirror(z, 96, 128, 0.5)
    assert 0 < len(kept) <= len(z)
