"""Cost of the scale NMS of the roots (pbd_set_scale_nms, k_scale_nms) on the bench workload -- 64 x 640x480 frames, person model --
and at the dense end, one 96 x 128 frame with every root cell eligible.

  cost       dl = 1, 2, 5, with and without pbd_set_root_nms(2): candidates found off / on, k_scale_nms next to k_grid_nms,
             k_top_k (K = 16) and k_argmin ms per step (event pairs on every launch, a run of their own), and end-to-end ms per
             step (host clock around steps that end in the read-back, profiling off), off and on, in alternating windows
  dense      one 96 x 128 frame, tiny model, thresh = -inf: every cell is eligible, so each wave scans 64 roots in turn

Prints one JSON line per measurement and appends them to profiles/scale_nms/probe.jsonl.

    python tools/probes/scale_nms_cost.py [cost|dense|all] [window_seconds]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from partsbaseddetector_amd import synth  # noqa: E402
from partsbaseddetector_amd.detector import PartsBasedDetector  # noqa: E402
from partsbaseddetector_amd.model import synthetic_person_model, synthetic_tiny_model  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
window = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
ROWS, COLS, K = 480, 640, 16
OUT = os.path.join(ROOT, "profiles", "scale_nms", "probe.jsonl")
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


def kernel_ms(hd, step):
    hd.profile(1)
    n, _ = timed_window(hd, step, window)
    prof = hd.profile_read()
    hd.profile(0)
    return {k: round(prof[k][0] / n, 4) for k in ("k_scale_nms", "k_grid_nms", "k_top_k", "k_argmin") if prof[k][1]}


def cost():
    B = 64
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
        for dl in (1, 2, 5):
            rec = {"probe": "cost", "dl": dl, "root_nms": sz, "workload": f"{B}x{COLS}x{ROWS}", "window_s": window,
                   "candidates": {}, "end_to_end_ms_per_step": {"off": [], "on": []}}
            for name, s in (("off", None), ("on", dl)):       # warm both settings; the counts
                hd.set_scale_nms(s)
                rec["candidates"][name] = step()
            for rnd in range(3):                              # end to end, profiling off, alternating windows
                for name, s in (("off", None), ("on", dl)):
                    hd.set_scale_nms(s)
                    rec["end_to_end_ms_per_step"][name].append(round(timed_window(hd, step, window)[1], 3))
            hd.set_scale_nms(dl)
            hd.set_top_k(K)                                   # k_top_k of the same run, over the survivors
            rec["candidates"]["on_top_k"] = step()
            rec["kernel_ms_per_step"] = kernel_ms(hd, step)
            hd.set_top_k(0)
            emit(rec)
    hd.set_scale_nms(None)
    hd.set_root_nms(0)
    hd.close()


def dense():
    det = PartsBasedDetector(device=0, max_batch=1, max_candidates=1 << 16)
    det.distributeModel(synthetic_tiny_model())
    hd = det.hd
    hd.set_thresh(-np.inf)
    d = torch.from_numpy(synth.synthetic_frame(5, 96, 128, 3)[None]).cuda()

    def step():
        _, n = det.detect_batch_device(d.data_ptr(), 1, 96, 128, 3, raw=True)
        return int(n)

    for dl in (1, 2, 5):
        hd.set_scale_nms(None)
        off = step()
        hd.set_scale_nms(dl)
        on = step()
        emit({"probe": "dense", "dl": dl, "workload": "1x128x96, thresh -inf", "candidates": {"off": off, "on": on},
              "kernel_ms_per_step": kernel_ms(hd, step)})
    hd.close()


if what in ("cost", "all"):
    cost()
if what in ("dense", "all"):
    dense()
