"""The cold variants of the resampling and HOG kernels, which bench.py does not run: per profile slot (k_resize, k_pyrdown,
k_hog_hist, k_hog_feat) the milliseconds of one call, median / min / max of --reps calls after --warmup calls.

CONFIGS rows are (depth, channels, real type, sbin, mixed).  A single-frame row is one 640x480 frame through detect(), the
equal-size entry (pbd_detect / pbd_detect_typed: k_resize<PT, Frames> or k_resize4, k_pyrdown<PT, Frames>); the mixed row is one
detect_frames() call of four small frames (pbd_detect_frames: k_resize<PT, Runs>, k_pyrdown<PT, Runs>).  The library is the one PBD_LIB names (two builds are compared by running the probe once per build, alternately).

    python tools/probes/feature_variants_cost.py --tag parent --out profiles/refactor_features/cold_variants.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from partsbaseddetector_amd import detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

CONFIGS = [("8U", 1, "f32", 8, False), ("8U", 3, "f64", 8, False), ("8U", 3, "f32", 6, False), ("16U", 3, "f32", 8, False),
           ("64F", 1, "f64", 4, False), ("8U", 3, "f32", 4, True)]
SMALL_MIX = [(160, 200), (96, 128), (121, 157), (100, 100)]        # tests/test_gpu_mixed_batch.py
DEPTHS = {"8U": np.uint8, "16U": np.uint16, "32F": np.float32, "64F": np.float64}
SLOTS = ("k_resize", "k_pyrdown", "k_hog_hist", "k_hog_feat")


def frame(seed, rows, cols, cn, depth):
    im = synth.synthetic_frame(seed, rows, cols, cn)
    return im if depth == "8U" else (im.astype(DEPTHS[depth]) * (257 if depth == "16U" else 1))


def measure(det, call, reps, warmup):
    for _ in range(warmup):
        call()
    ms = {k: [] for k in SLOTS}
    for _ in range(reps):
        det.hd.profile(True)
        call()
        prof = det.hd.profile_read()
        det.hd.profile(False)
        for k in SLOTS:
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
    for depth, cn, real, sbin, mixed in CONFIGS:
        model = M.synthetic_model(seed=7, pa=[0, 1], nmix=1, ksize=3, sbin=sbin, interval=10, thresh=1e9, name="front-end")
        det = detector.PartsBasedDetector(device=0, max_batch=4, dtype=np.float32 if real == "f32" else np.float64)
        det.distributeModel(model)
        if mixed:
            frames = [frame(40 + i, r, c, cn, depth) for i, (r, c) in enumerate(SMALL_MIX)]
        else:
            frames = [frame(40, 480, 640, cn, depth)]
        res = measure(det, (lambda: det.detect_frames(frames)) if mixed else (lambda: det.detect(frames[0])), args.reps, args.warmup)
        det.hd.close()
        lines.append(json.dumps({"tag": args.tag, "config": "mixed SMALL_MIX" if mixed else "640x480", "depth": depth, "cn": cn,
                                 "real": real, "sbin": sbin, "reps": args.reps, "slots": res}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
