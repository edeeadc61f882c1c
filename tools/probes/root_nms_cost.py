"""Cost of the root NMS (pbd_set_root_nms, k_grid_nms) on the bench workload: 64 x 640x480 frames, person model.

  variants   k_grid_nms with one lane and with one wave per block (pbd_debug_set_option, GRID_NMS_LANES) at a row of window
             sizes: the resident result is re-emitted (pbd_argmin_device_out: grid NMS, find, walk) in alternating windows of at
             least 0.5 s each, every launch timed by its own event pair; ms per launch of k_grid_nms per window.  This is the
             measurement that places kGnWaveSz (pbd_internal.h).
  cost       for sz in 1, 2, 4, 8: candidates found off / on, k_grid_nms and k_argmin ms per step (event pairs, a run of their
             own), and end-to-end ms per step (host clock around steps that end in the read-back, profiling off), off and on,
             each with and without pbd_set_nms(0.1), in alternating windows of one process.

Prints one JSON line per measurement and appends them to profiles/grid_nms/probe.jsonl.

    python tools/probes/root_nms_cost.py [variants|cost|all] [window_seconds]"""
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

what = sys.argv[1] if len(sys.argv) > 1 else "all"
window = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
ROWS, COLS, B = 480, 640, 64
OUT = os.path.join(ROOT, "profiles", "grid_nms", "probe.jsonl")
os.makedirs(os.path.dirname(OUT), exist_ok=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16)
det.distributeModel(synthetic_person_model())
hd = det.hd
d = torch.from_numpy(np.stack([synth.synthetic_frame(i + 1, ROWS, COLS, 3) for i in range(B)])).cuda()
cap = 1 << 16
pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")


def step():
    _, n = det.detect_batch_device(d.data_ptr(), B, ROWS, COLS, 3, raw=True)
    return int(n)


def timed_window(fn, seconds):
    """calls of fn for at least `seconds`, ending in a synchronise: (calls, wall ms per call).  With profiling on, the event pairs
    are folded into the handle's totals every 64 calls, so their number stays bounded"""
    torch.cuda.synchronize()
    hd.check(hd.lib.pbd_synchronize(hd.h))
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        if n % 8 == 0 or seconds <= 0:
            hd.check(hd.lib.pbd_synchronize(hd.h))
            if n % 64 == 0:
                hd.check(hd.lib.pbd_profile_read(hd.h, 0, None, None))
            if time.perf_counter() - t0 >= seconds:
                break
    hd.check(hd.lib.pbd_synchronize(hd.h))
    return n, (time.perf_counter() - t0) * 1e3 / n


step()                                                    # plans, workspaces; the result stays resident
if what in ("variants", "all"):
    for sz in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 32):
        hd.set_root_nms(sz)
        rec = {"probe": "variants", "sz": sz, "window_s": window, "k_grid_nms_ms": {1: [], 64: []}, "launches": {1: [], 64: []}}
        for lanes in (1, 64):                             # warm both
            hd.set_debug_option(_lib.GRID_NMS_LANES, lanes)
            det.argmin_device_out(0, pay.data_ptr(), cap)
        for rnd in range(3):
            for lanes in (1, 64):
                hd.set_debug_option(_lib.GRID_NMS_LANES, lanes)
                hd.profile(1)
                timed_window(lambda: det.argmin_device_out(0, pay.data_ptr(), cap), window)
                ms, n = hd.profile_read()["k_grid_nms"]
                hd.profile(0)
                rec["k_grid_nms_ms"][lanes].append(round(ms / max(n, 1), 5))
                rec["launches"][lanes].append(n)
        rec["kept"] = int(pay[0].item())
        emit(rec)
    hd.set_debug_option(_lib.GRID_NMS_LANES, 0)
    hd.set_root_nms(0)

if what in ("cost", "all"):
    for sz in (1, 2, 4, 8):
        rec = {"probe": "cost", "sz": sz, "workload": f"{B}x{COLS}x{ROWS}", "window_s": window}
        for nms in (None, 0.1):
            tag = "nms0.1" if nms is not None else "raw"
            hd.set_nms(nms)
            out = {"candidates": {}, "k_grid_nms_ms_per_step": None, "k_argmin_ms_per_step": {}, "end_to_end_ms_per_step": {"off": [], "on": []}}
            for name, s in (("off", 0), ("on", sz)):      # warm both settings; the counts
                hd.set_root_nms(s)
                out["candidates"][name] = step()
            for rnd in range(3):                          # end to end, profiling off, alternating windows
                for name, s in (("off", 0), ("on", sz)):
                    hd.set_root_nms(s)
                    out["end_to_end_ms_per_step"][name].append(round(timed_window(step, window)[1], 3))
            for name, s in (("off", 0), ("on", sz)):      # kernel times: event pairs on every launch, a run of their own
                hd.set_root_nms(s)
                hd.profile(1)
                n, _ = timed_window(step, window)
                prof = hd.profile_read()
                hd.profile(0)
                out["k_argmin_ms_per_step"][name] = round(prof["k_argmin"][0] / n, 4)
                if s:
                    out["k_grid_nms_ms_per_step"] = round(prof["k_grid_nms"][0] / n, 4)
            rec[tag] = out
        emit(rec)
    hd.set_nms(None)
    hd.set_root_nms(0)
hd.close()
