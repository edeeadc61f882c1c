"""Cost of pbd_max_marginals and pbd_marginal_poses_device on one 640x480 frame, synthetic person model (26 parts x 6 types:
150 upward and 900 mirrored transforms).  In one process, alternating: a detect call of the frame (profiled: the dynamic program's
own kernels from pbd_profile_read) and pbd_max_marginals (timed between two events on the handle's stream without profiling, then
once more with profiling for the per-kernel split under the k_mm_* ids).  Then the decode of 1 seed and of 1000 seeds, timed the
same way.  The device memory the call holds is read as the drop of free device memory across the first call.  One JSON line per
real type; with an argument, also written to that file.

    python tools/probes/marginals_cost.py [out.jsonl] [--reps N]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

ROWS, COLS = 480, 640
DP = ("k_dt_rows", "k_dt_cols", "k_dp_combine", "k_dp_root")


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    import torch
    torch.cuda.init()
    args = [a for a in sys.argv[1:]]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 9
    path = args[0] if args and not args[0].startswith("--") else None
    im = synth.synthetic_frame(1, ROWS, COLS)
    out = []
    for dtype in (np.float32, np.float64):
        det = detector.PartsBasedDetector(device=0, max_candidates=1 << 16, dtype=dtype)
        det.distributeModel(M.synthetic_person_model())
        hd = det.hd
        stream = torch.cuda.ExternalStream(hd.stream_ptr(), device="cuda:0")

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        det.detect(im)
        free0 = torch.cuda.mem_get_info()[0]
        hd.max_marginals(0)
        hd.check(hd.lib.pbd_synchronize(hd.h))
        held = free0 - torch.cuda.mem_get_info()[0]
        dp_ms, mm_ms = [], []
        for _ in range(reps):
            hd.profile(True)
            det.detect(im)
            pr = hd.profile_read()
            hd.profile(False)
            dp_ms.append(sum(pr[k][0] for k in DP))
            mm_ms.append(timed(lambda: hd.max_marginals(0)))
        hd.profile(True)
        hd.max_marginals(0)
        pr = hd.profile_read()
        hd.profile(False)
        split = {k: {"ms": round(pr[k][0], 4), "launches": pr[k][1]} for k in _lib.KERNELS_MM if pr[k][1]}
        # seeds: the best cells of part 13 on level 0
        shapes = hd.level_shapes
        H, W = shapes[0]
        rng = np.random.default_rng(1)
        seeds = np.stack([np.zeros(1000, np.int32), np.zeros(1000, np.int32), rng.integers(0, 26, 1000).astype(np.int32),
                          np.full(1000, -1, np.int32), rng.integers(0, W, 1000).astype(np.int32), rng.integers(0, H, 1000).astype(np.int32)], 1)
        d_seeds = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
        d_rec = torch.zeros((1000, hd.stride), dtype=torch.int32, device="cuda")
        d_status = torch.zeros(1000, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pose = {}
        for n in (1, 1000):
            call = lambda: hd.marginal_poses_device(n, d_seeds.data_ptr(), None, 0, d_rec.data_ptr(), None, d_status.data_ptr())
            for _ in range(3):
                timed(call)
            pose[n] = stats([timed(call) for _ in range(reps)])
        assert int((d_status.cpu().numpy() == 26).sum()) == 1000
        cells = sum(r * c for r, c in shapes)
        res = {"T": np.dtype(dtype).name, "cells": cells, "levels": len(shapes), "reps": reps, "dp_ms": stats(dp_ms),
               "max_marginals_ms": stats(mm_ms), "ratio": round(float(np.median(mm_ms) / np.median(dp_ms)), 2), "split": split,
               "held_bytes": int(held), "poses_1_ms": pose[1], "poses_1000_ms": pose[1000]}
        print(json.dumps(res))
        out.append(res)
        hd.close()
    if path:
        with open(path, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
