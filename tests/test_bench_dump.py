"""bench.py --dump-outputs: the candidate records of the last timed step, written field by field as .npy (float32 /
float64), capped at 64 MB by a fixed seeded sample; and --steps / --warmup refused when they cannot be honoured."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(n, max_parts, seed=5):
    rng = np.random.default_rng(seed)
    rec = rng.integers(-1000, 1000, size=(n, 8 + 4 * max_parts)).astype(np.int32)      # unused part slots hold junk
    rec[:, 0] = np.arange(n) // 3
    rec[:, 5] = rng.standard_normal(n).astype(np.float32).view(np.int32)
    rec[:, 6] = rng.integers(1, max_parts + 1, size=n)
    return rec


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_field(tmp_path):
    rec = _records(7, 3)
    shapes = bench.dump_outputs(str(tmp_path), rec)
    got = _load(str(tmp_path))
    assert set(got) == set(shapes) == {"candidate_header", "candidate_score", "candidate_parts", "candidate_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["candidate_header"], rec[:, [0, 1, 2, 3, 4, 6]].astype(np.float64))
    assert np.array_equal(got["candidate_score"].view(np.int32), rec[:, 5])
    assert np.array_equal(got["candidate_rows"], np.arange(7))
    for i in range(7):
        k = rec[i, 6]
        assert np.array_equal(got["candidate_parts"][i, :k], rec[i, 8:8 + 4 * k].reshape(k, 4))
        assert not got["candidate_parts"][i, k:].any()


def test_dump_of_an_empty_list(tmp_path):
    bench.dump_outputs(str(tmp_path), np.zeros((0, 20), np.int32))
    got = _load(str(tmp_path))
    assert got["candidate_header"].shape == (0, 6) and got["candidate_parts"].shape == (0, 3, 4)


def test_dump_is_capped_by_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    rec = _records(200, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rec)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(x.nbytes for x in a.values()) <= 4096
    rows = a["candidate_rows"].astype(np.int64)
    assert 0 < len(rows) < 200 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["candidate_header"], rec[rows][:, [0, 1, 2, 3, 4, 6]].astype(np.float64))
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_steps_and_warmup_are_checked():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and bad[0] in r.stderr, r.stderr
