"""Time of pbd_cluster_parts_device at sizes a user would run -- the 26-part person tree, K = 6, R = 100 trials, N = 1 000 and
10 000 positives -- measured with device events over a warmed-up window of at least half a second, with the two kernels' shares
from pbd_profile_read, next to the numpy yardstick (trainmodel.cluster_parts_ref) on the same host.  The yardstick is timed on
REF_TRIALS trials per part (its cost per trial does not depend on the number of trials) and the figure for R = 100 is that time
scaled, marked as such; the device is also run at REF_TRIALS and compared with it bit for bit.  Prints one JSON line per size;
with an argument, also writes them to that file.

    python tools/probes/cluster_parts_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402
from partsbaseddetector_amd import trainmodel as TM  # noqa: E402

P, K, R, REF_TRIALS, WINDOW_S = 26, 6, 100, 2, 0.5


def person_def(n, seed=1):
    """(26, n, 2): every part its parent's position plus one of six offsets (cells) and unit noise"""
    rng = np.random.default_rng(seed)
    parent = TM.parent_of(synth.PERSON_PA)
    d = np.zeros((P, n, 2))
    d[0] = rng.normal(size=(n, 2)) * 3
    for p in range(1, P):
        centres = rng.normal(size=(K, 2)) * 4
        d[p] = d[parent[p]] + centres[rng.integers(0, K, n)] + rng.normal(size=(n, 2))
    return d, parent


def main():
    import torch
    torch.cuda.init()
    hd = detector.Handle(M.synthetic_tiny_model())
    out = []
    for n in (1000, 10000):
        d, parent = person_def(n)
        Ks = [K] * P
        t_def = torch.from_numpy(d).cuda()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        idx, cen, cnt, anc = z((P, n), torch.int32), z((P, 16, 2), torch.float64), z((P, 16), torch.int32), z((P, 16, 2), torch.int32)
        info, its = z((P, 16), torch.uint8), z((P, R), torch.int32)

        def call(trials=R):
            hd.cluster_parts_device(P, n, t_def.data_ptr(), parent, Ks, trials, 1000, 0, idx.data_ptr(), cen.data_ptr(), cnt.data_ptr(),
                                    anc.data_ptr(), info.data_ptr(), None, its.data_ptr())

        stream = torch.cuda.ExternalStream(hd.stream_ptr())
        for _ in range(2):
            call()
        hd.check(hd.lib.pbd_synchronize(hd.h))
        reps, ms = 1, 0.0
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                call()
            b.record(stream)
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= WINDOW_S * 1e3:
                break
            reps = max(reps * 2, int(reps * WINDOW_S * 1e3 / max(ms, 1e-3)) + 1)
        iters = its.cpu().numpy()
        hd.profile(True)
        call()
        hd.check(hd.lib.pbd_synchronize(hd.h))
        prof = hd.profile_read()
        hd.profile(False)
        # the yardstick, and the device against it, at REF_TRIALS trials per part
        t0 = time.perf_counter()
        want = TM.cluster_parts_ref(d, parent, Ks, REF_TRIALS, 1000, 0)
        ref_s = time.perf_counter() - t0
        got = hd.cluster_parts(d, parent, Ks, REF_TRIALS, 1000, 0)
        equal = all(np.array_equal(got[k], want[k]) for k in ("idx", "counts", "anchors", "iters_all", "info")) and \
            got["sumdist_all"].tobytes() == want["sumdist_all"].tobytes()
        rec = {"case": f"P {P}, K {K}, R {R}, N {n}", "calls_in_window": reps, "window_ms": round(ms, 1),
               "device_ms_per_call": round(ms / reps, 3),
               "kernel_ms": {k: round(prof[k][0], 3) for k in ("k_km_trials", "k_km_pick")},
               "iterations_mean_max": [round(float(iters.mean()), 1), int(iters.max())],
               "ref_trials": REF_TRIALS, "ref_s_measured": round(ref_s, 2), "ref_s_scaled_to_R": round(ref_s * R / REF_TRIALS, 1),
               "ref_iterations_mean": round(float(want["iters_all"].mean()), 1), "equals_ref_at_ref_trials": bool(equal)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
