"""The cold variants of the dynamic program's kernels, which bench.py does not run: per profile slot (k_dt_rows, k_dt_cols,
k_dp_combine, k_dp_root, k_argmin; k_ex_walk for the examples row) the milliseconds of one call, median / min / max of --reps
calls after --warmup calls, on the synthetic person model.

CONFIGS rows are (name, frame sizes, real type, conv mode).  One 640x480 frame through detect() takes the narrow waves and the
cooperative kernel k_dt_coop (float), the narrow k_dt_pass<double, ...> (double) or the fp16-response rows pass and combine
(f16); one 1920x1080 frame has int16 position planes and NARROW waves; the mixed row is one detect_frames() call of four small
frames; the examples row times pbd_examples on the records of the 640x480 frame.  The library is the one PBD_LIB names (two
builds are compared by running the probe once per build, alternately).

    python tools/probes/dp_variants_cost.py --tag parent --out profiles/refactor_dp/cold_variants.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

SMALL_MIX = [(160, 200), (96, 128), (121, 157), (100, 100)]        # tests/test_gpu_mixed_batch.py
CONFIGS = [("640x480", [(480, 640)], "f32", _lib.CONV_EXACT), ("640x480", [(480, 640)], "f64", _lib.CONV_EXACT),
           ("640x480 fp16 responses", [(480, 640)], "f32", _lib.CONV_MFMA_F16), ("1920x1080", [(1080, 1920)], "f32", _lib.CONV_EXACT),
           ("mixed SMALL_MIX", SMALL_MIX, "f32", _lib.CONV_EXACT), ("examples 640x480", [(480, 640)], "f32", _lib.CONV_EXACT)]
DP_SLOTS = ("k_dt_rows", "k_dt_cols", "k_dp_combine", "k_dp_root", "k_argmin")


def measure(det, call, slots, reps, warmup):
    for _ in range(warmup):
        call()
    ms = {k: [] for k in slots}
    for _ in range(reps):
        det.hd.profile(True)
        call()
        prof = det.hd.profile_read()
        det.hd.profile(False)
        for k in slots:
            ms[k].append(prof[k][0])
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name, sizes, real, conv in CONFIGS:
        det = detector.PartsBasedDetector(device=0, conv_mode=conv, max_batch=4, dtype=np.float32 if real == "f32" else np.float64)
        det.distributeModel(M.synthetic_person_model(thresh=M.PERSON_THRESH - 1.0))
        frames = [synth.synthetic_frame(40 + i, r, c) for i, (r, c) in enumerate(sizes)]
        if name.startswith("examples"):
            cands = det.detect(frames[0])
            res = measure(det, lambda: det.examples(cands), ("k_ex_walk", "k_ex_gather"), args.reps, args.warmup)
            res["records"] = len(cands)
        else:
            res = measure(det, (lambda: det.detect_frames(frames)) if len(frames) > 1 else (lambda: det.detect(frames[0])), DP_SLOTS,
                          args.reps, args.warmup)
        det.hd.close()
        lines.append(json.dumps({"tag": args.tag, "config": name, "real": real, "reps": args.reps, "slots": res}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
