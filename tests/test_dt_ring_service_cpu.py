"""The whole-wave ring service of the streamed distance transform (DtRing::push_below / service_reload / pop in
pbd_kernels_dp.hip) replayed on the CPU with the shipped thresholds (tests/dt_wave_replay.py): 64 lanes in lock step, entries
moved between registers, ring and spill stack as the kernel moves them.  On the planes tests/test_gpu_dt_ring_service.py gives
the GPU -- rows of one wave at different depths: constant, pop-all ramp, spikes, quantised, noise and staircases of 8 to 11
entries -- every lane's finished envelope (v, z) and every read-out (value, pointer) must equal plain computeRow bit for bit, no
service may break an invariant it relies on (even lo, room for a pair, no reload with lo == 0, the host's stack records: the
replay asserts them where it serves), and the inputs must reach the events the service is made of."""
import os
import re

import numpy as np
import pytest

import dt_hard_planes as H
import dt_wave_replay as W

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "partsbaseddetector_amd", "csrc", "pbd_kernels_dp.hip")


def test_replay_uses_the_shipped_thresholds():
    text = open(SRC).read()
    shipped = {name: int(re.search(r"#define %s (-?\d+)" % name, text).group(1))
               for name in ("PBD_DT_RING", "PBD_DT_HIGH", "PBD_DT_LOW", "PBD_DT_LOW_RO", "PBD_DT_CH", "PBD_DT_CHC")}
    assert shipped == {"PBD_DT_RING": W.T_RING, "PBD_DT_HIGH": W.HIGH, "PBD_DT_LOW": W.LOW, "PBD_DT_LOW_RO": W.LOW_RO,
                       "PBD_DT_CH": W.CHUNK, "PBD_DT_CHC": W.CHUNK}


def test_staircase_rows_reach_their_depths():
    """The envelope of staircase row s is 8 + s entries deep at the end of every step, and each riser pops the whole step."""
    rng = np.random.default_rng(0)
    rows = np.stack([W._row(f"stairs{s}", rng, 64, 0) for s in range(4)])
    st = H.replay_rows(rows, -0.01, -0.0, 0)[2]
    assert st["depth"].tolist() == [8, 9, 10, 11] and st["maxpop"].tolist() == [7, 8, 9, 10]
    for s in range(4):
        ends = [(7 + s) * j + 1 for j in range(1, 5)]
        assert [int(W.plain_rows(rows[s:s + 1, :n], -0.01, -0.0, 0)[2][0]) + 1 for n in ends] == [8 + s] * 4


@pytest.mark.parametrize("set_name", list(W.SIZES))
@pytest.mark.parametrize("deformation", ["default", "linear"])
@pytest.mark.parametrize("real", ["f32", "f64"])
def test_service_replay_equals_compute_row(real, deformation, set_name):
    R = np.float64 if real == "f64" else np.float32
    flat = H.dt_model("tiny", deformation).flatten()
    levels = W.service_levels(flat.nfilters, set_name, 303, np.float64 if real == "f64" else np.float32)
    jobs = H.leaf_jobs(flat)
    rows_c, cols_c = W.new_counts(), W.new_counts()
    for f, ax, bx, ay, by, osx, osy in (jobs[0], jobs[-1]):
        tmp, _ = W.replay_levels([l[f] for l in levels], ax, bx, osx, R, counts=rows_c)      # asserts equality with computeRow
        W.replay_levels([t.T for t in tmp], ay, by, osy, R, counts=cols_c)
    for pas, c in (("rows", rows_c), ("cols", cols_c)):
        print(real, deformation, set_name, pas, c)
    c = {k: rows_c[k] + cols_c[k] for k in rows_c}
    assert c["a_high_joins_high_minus_1_stays"] > 0       # (a) a lane at HIGH spills for another's overflow, one at HIGH - 1 stays
    assert c["b_lo0_bystander"] > 0                       # (b) a lane with lo == 0 and few entries sits a whole-wave reload out
    assert c["c_fwd_service_joined"] > 0                  # (c) whole-wave reload in the forward scan, more lanes than the drained one
    assert c["d_ro_service_joined"] > 0                   # (d) ... in the read-out
    assert c["fallback_fwd"] > 0                          # (e) more pops in one element than the ring holds: pop()'s own reload
    if set_name == "u8":
        assert rows_c["fallback_ro"] + cols_c["fallback_ro"] > 0


def test_lane_by_lane_policy_is_the_same_transform():
    """The service's thresholds at their off positions (every lane for itself) give the same envelopes and read-outs."""
    flat = H.dt_model("tiny", "default").flatten()
    levels = W.service_levels(flat.nfilters, "i16", 303)
    f, ax, bx, _, _, osx, _ = H.leaf_jobs(flat)[0]
    _, c = W.replay_levels([l[f] for l in levels], ax, bx, osx, np.float32, **W.LANE_BY_LANE)
    assert c["service_fwd"] == c["service_ro"] == 0 and c["fallback_ro"] > 0 and c["spill_paths"] > 0
