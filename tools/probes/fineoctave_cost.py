"""Cost of the fine octave (pbd_set_fine_octave): person model, 16 resident 640x480 frames, PBD_CONV_EXACT and
PBD_CONV_MFMA, one process.

Per mode two handles, one with the octave off and one with it on, take turns: three rounds of a timed window each, profiling off,
every window ending in a device synchronisation -> ms per step.  Then one window each with an event pair on every launch -> ms
per step of every kernel (pbd_profile_read).  Cells per frame are counted from pbd_pyramid_plan.

The one comparison that justifies k_hog_tile<2>: a third handle with the octave on and the histogram stage forced onto the two-pass
form (k_hog_grad4 once over the level images, then the ranged k_hog_hist per bin size), same frames, same windows; its
k_hog_hist column against the fused handle's is the time of the two forms over the SAME levels (both bin sizes).

Prints one JSON line per mode, appends it to profiles/fineoctave/probe.jsonl, and prints the markdown table of
profiles/fineoctave/README.md.

    python tools/probes/fineoctave_cost.py [window_seconds]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from partsbaseddetector_amd import _lib, synth  # noqa: E402
from partsbaseddetector_amd.detector import PartsBasedDetector  # noqa: E402
from partsbaseddetector_amd.model import synthetic_person_model  # noqa: E402

window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
ROWS, COLS, B = 480, 640, 16
OUT = os.path.join(ROOT, "profiles", "fineoctave", "probe.jsonl")
os.makedirs(os.path.dirname(OUT), exist_ok=True)

model = synthetic_person_model()
d = torch.from_numpy(np.stack([synth.synthetic_frame(i + 1, ROWS, COLS, 3) for i in range(B)])).cuda()
torch.cuda.synchronize()


def timed_window(det, seconds):
    """steps of det for at least `seconds`, ending in a synchronise: (steps, wall ms per step)"""
    hd = det.hd
    hd.check(hd.lib.pbd_synchronize(hd.h))
    t0, n = time.perf_counter(), 0
    while True:
        det.detect_batch_device(d.data_ptr(), B, ROWS, COLS, 3, raw=True)
        n += 1
        if n % 16 == 0:
            hd.check(hd.lib.pbd_profile_read(hd.h, 0, None, None))   # folds the event pairs of a profiled window
        if time.perf_counter() - t0 >= seconds:
            break
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return n, (time.perf_counter() - t0) * 1e3 / n


NAMES = ("off", "on", "on-two-pass")
rows = []
for mode_name, mode in (("exact", _lib.CONV_EXACT), ("mfma", _lib.CONV_MFMA)):
    dets = {}
    for name in NAMES:
        det = PartsBasedDetector(device=0, conv_mode=mode, max_batch=B, max_candidates=1 << 19)
        det.setFineOctave(name != "off")
        det.distributeModel(model)
        if name == "on-two-pass":
            det.hd.set_debug_option(_lib.HOG_TWO_PASS, 1)
        dets[name] = det
    rec = {"probe": "fineoctave_cost", "mode": mode_name, "workload": f"{B}x{COLS}x{ROWS}", "window_s": window, "levels": {},
           "cells_per_frame": {}, "candidates": {}, "ms_per_step": {n: [] for n in NAMES}, "kernel_ms_per_step": {}}
    for name, det in dets.items():
        plan = det.hd.plan(ROWS, COLS)
        rec["levels"][name] = int(plan["nlevels"])
        rec["cells_per_frame"][name] = int((plan["feat_rows"].astype(np.int64) * plan["feat_cols"]).sum())
        _, n = det.detect_batch_device(d.data_ptr(), B, ROWS, COLS, 3, raw=True)          # warm: plans, workspaces
        rec["candidates"][name] = int(n)
    for rnd in range(3):
        for name, det in dets.items():
            rec["ms_per_step"][name].append(round(timed_window(det, window)[1], 3))
    for name, det in dets.items():
        det.hd.profile(1)
        n, _ = timed_window(det, window)
        prof = det.hd.profile_read()
        det.hd.profile(0)
        rec["kernel_ms_per_step"][name] = {k: round(ms / n, 4) for k, (ms, _) in prof.items() if ms > 0}
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    rows.append(rec)
    for det in dets.values():
        det.hd.close()

print()
kernels = sorted({k for r in rows for v in r["kernel_ms_per_step"].values() for k in v})
print("| mode | octave | levels | cells / frame | candidates / step | ms / step (3 windows) | " + " | ".join(f"`{k}`" for k in kernels) + " |")
print("|---" * (6 + len(kernels)) + "|")
for r in rows:
    for name in NAMES:
        ks = r["kernel_ms_per_step"][name]
        print(f"| {r['mode']} | {name} | {r['levels'][name]} | {r['cells_per_frame'][name]} | {r['candidates'][name]} | "
              f"{' / '.join(str(v) for v in r['ms_per_step'][name])} | " + " | ".join(str(ks.get(k, '')) for k in kernels) + " |")
