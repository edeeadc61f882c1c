"""Cost of the per-frame top-K of the roots (pbd_set_top_k, k_top_k) on the bench workload -- 64 x 640x480 frames, person model --
and on one 640x480 frame per step.

  cost       K = 16, with and without pbd_set_root_nms(2): candidates found off / on, k_top_k, k_grid_nms and k_argmin ms per step
             and the launches of k_top_k per step (event pairs on every launch, a run of their own), and end-to-end ms per step
             (host clock around steps that end in the read-back, profiling off), off and on, in alternating windows of one process
  single     the same for a batch of one frame: there the launch count matters more than the bytes
  data       k_top_k ms per call of pbd_top_k_cells_device over 64 segments of the bench workload's frame length for random,
             all-equal and shared-upper-bits values and K = 16 and K above the length: the cost must not depend on the data

Prints one JSON line per measurement and appends them to profiles/top_k/probe.jsonl.

    python tools/probes/top_k_cost.py [cost|single|data|all] [window_seconds]"""
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
ROWS, COLS, K = 480, 640, 16
OUT = os.path.join(ROOT, "profiles", "top_k", "probe.jsonl")
os.makedirs(os.path.dirname(OUT), exist_ok=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def timed_window(hd, fn, seconds):
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


def cost(B, probe):
    det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16)
    det.distributeModel(synthetic_person_model())
    hd = det.hd
    d = torch.from_numpy(np.stack([synth.synthetic_frame(i + 1, ROWS, COLS, 3) for i in range(B)])).cuda()

    def step():
        _, n = det.detect_batch_device(d.data_ptr(), B, ROWS, COLS, 3, raw=True)
        return int(n)

    step()
    for sz in (0, 2):
        hd.set_root_nms(sz)
        rec = {"probe": probe, "k": K, "root_nms": sz, "workload": f"{B}x{COLS}x{ROWS}", "window_s": window, "candidates": {},
               "end_to_end_ms_per_step": {"off": [], "on": []}, "k_argmin_ms_per_step": {}, "k_grid_nms_ms_per_step": {}}
        for name, k in (("off", 0), ("on", K)):           # warm both settings; the counts
            hd.set_top_k(k)
            rec["candidates"][name] = step()
        for rnd in range(3):                              # end to end, profiling off, alternating windows
            for name, k in (("off", 0), ("on", K)):
                hd.set_top_k(k)
                rec["end_to_end_ms_per_step"][name].append(round(timed_window(hd, step, window)[1], 3))
        for name, k in (("off", 0), ("on", K)):           # kernel times: event pairs on every launch, a run of their own
            hd.set_top_k(k)
            hd.profile(1)
            n, _ = timed_window(hd, step, window)
            prof = hd.profile_read()
            hd.profile(0)
            rec["k_argmin_ms_per_step"][name] = round(prof["k_argmin"][0] / n, 4)
            rec["k_grid_nms_ms_per_step"][name] = round(prof["k_grid_nms"][0] / n, 4)
            if k:
                rec["k_top_k_ms_per_step"] = round(prof["k_top_k"][0] / n, 4)
                rec["k_top_k_launches_per_step"] = round(prof["k_top_k"][1] / n, 2)
        emit(rec)
    hd.set_top_k(0)
    hd.set_root_nms(0)
    return det


def data(det):
    hd = det.hd
    n, nseg = 141_000, 64                                 # about one VGA frame's root cells per segment
    rng = np.random.default_rng(1)
    inputs = {"random": rng.standard_normal(n * nseg).astype(np.float32),
              "all_equal": np.full(n * nseg, 1.5, np.float32),
              "shared_upper_24_bits": (np.uint32(0x3FC00000) | rng.integers(0, 256, n * nseg).astype(np.uint32)).view(np.float32)}
    dst = torch.zeros(n * nseg, dtype=torch.uint8, device="cuda")
    for name, v in inputs.items():
        src = torch.from_numpy(v).cuda()
        for k in (K, n + 1):
            call = lambda: hd.top_k_cells_device([n] * nseg, _lib.REAL_F32, src.data_ptr(), None, k, dst.data_ptr())
            call()
            hd.profile(1)
            calls, _ = timed_window(hd, call, window)
            ms, launches = hd.profile_read()["k_top_k"]
            hd.profile(0)
            emit({"probe": "data", "values": name, "k": k, "segments": nseg, "length": n,
                  "k_top_k_ms_per_call": round(ms / calls, 4), "launches_per_call": round(launches / calls, 2),
                  "kept": int((dst != 0).sum().item())})


det = None
if what in ("cost", "all"):
    det = cost(64, "cost")
if what in ("data", "all"):
    if det is None:
        det = PartsBasedDetector(device=0, max_batch=1)
        det.distributeModel(synthetic_person_model())
    data(det)
if det is not None:
    det.hd.close()
if what in ("single", "all"):
    cost(1, "single").hd.close()
