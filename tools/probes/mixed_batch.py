"""Mixed-size frames: one pbd_detect_frames call against one pbd_detect_batch per size and one pbd_detect per frame.

Person model, exact float, the mix {1 x 1920x1080, 2 x 1280x720, 4 x 640x480, 8 x 320x240} (15 frames).  The three ways run
alternately in one process after a warm-up; every repetition is one wall-clock time of a synchronous host call sequence.
Also: the host time of the first call with a size list the handle has not seen (no size of it planned before: the per-size
tables and the mixed plan built, the mixed plan uploaded) against the same call once the plan is cached.

    python tools/probes/mixed_batch.py --reps 25 --out profiles/mixed_batch/probe.json
    python tools/probes/mixed_batch.py --only a --reps 3      # one way only (kernel traces)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

MIX = [(1080, 1920)] + [(720, 1280)] * 2 + [(480, 640)] * 4 + [(240, 320)] * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    hd = detector.Handle(M.synthetic_person_model(), max_batch=16, max_candidates=1 << 18)
    frames = [synth.synthetic_frame(31 + i, r, c, 3) for i, (r, c) in enumerate(MIX)]
    cap = hd.max_candidates
    buf = np.zeros(cap * hd.stride, np.int32)
    n = C.c_int()

    def descs(fr):
        return _lib.frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr])

    def way_a():
        hd.check(hd.lib.pbd_detect_frames(hd.h, len(frames), descs(frames), 3, 0, buf.ctypes.data, cap, C.byref(n)))
        return n.value

    by_size = {}
    for f in frames:
        by_size.setdefault(f.shape, []).append(f)

    def way_b():
        tot = 0
        for (r, c, cn), fr in by_size.items():
            hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), r, c, cn, c * cn, buf.ctypes.data, cap, C.byref(n)))
            tot += n.value
        return tot

    def way_c():
        tot = 0
        for f in frames:
            hd.check(hd.lib.pbd_detect(hd.h, f.ctypes.data, f.shape[0], f.shape[1], 3, f.strides[0], buf.ctypes.data, cap, C.byref(n)))
            tot += n.value
        return tot

    ways = {"a": way_a, "b": way_b, "c": way_c}
    if args.only:
        ways = {args.only: ways[args.only]}
    counts = {k: fn() for k, fn in ways.items()}
    if len(ways) == 3:
        assert counts["a"] == counts["b"] == counts["c"], counts
    for _ in range(args.warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(args.reps):
        for k, fn in ways.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"mix": [list(s) for s in MIX], "frames": len(MIX), "candidates": counts, "reps": args.reps}
    for k, t in times.items():
        t = np.array(t)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90))}

    if args.only is None:
        # first call with an unseen size list, as a tracker whose regions change size on every call sees it: every frame
        # cropped by 1 + k pixels, so that no size of the list has been planned before (mixed plan AND per-size tables built)
        first, again = [], []
        for k in range(5):
            crop = [np.ascontiguousarray(f[: f.shape[0] - 1 - k, : f.shape[1] - 1 - k]) for f in frames]
            t0 = time.perf_counter()
            hd.check(hd.lib.pbd_detect_frames(hd.h, len(crop), descs(crop), 3, 0, buf.ctypes.data, cap, C.byref(n)))
            first.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            hd.check(hd.lib.pbd_detect_frames(hd.h, len(crop), descs(crop), 3, 0, buf.ctypes.data, cap, C.byref(n)))
            again.append((time.perf_counter() - t0) * 1e3)
        res["unseen_size_list"] = {"first_call_ms": first, "cached_call_ms": again,
                                   "plan_build_ms_median": float(np.median(np.array(first) - np.array(again)))}
    hd.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
