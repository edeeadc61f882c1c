"""Cost of the scale-depth pruning (pbd_set_depth_prune + pbd_bind_depth_device, k_depth_prune) on the bench workload: 64 x 640x480
frames, person model, its threshold.

The depth scene is synthetic and built from a seed: a ground plane that recedes from 1 m at the bottom row to 6 m at the top, and
twelve boxes standing at 0.8 .. 4.5 m, with 3 % holes; one image per frame, in millimetres as 16U and in metres as 32F.  The rule's
parameters: fx = 525 pixels, a root footprint 0.45 m wide, tol = 0.3.

For each depth type: candidates found off / on, k_depth_prune and k_argmin ms per step (event pairs on every launch, a run of their
own), and end-to-end ms per step (host clock around steps that end in the read-back, profiling off) off and on, each with and
without pbd_set_nms(0.1), in alternating windows of one process.  A step with pruning on includes its pbd_bind_depth_device call.

Prints one JSON line per measurement and appends them to profiles/depth_prune/probe.jsonl.

    python tools/probes/depth_prune_cost.py [window_seconds] [seed]"""
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
from partsbaseddetector_amd.model import synthetic_person_model  # noqa: E402

window = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
ROWS, COLS, B = 480, 640, 64
FX, WIDTH_M, TOL = 525.0, 0.45, 0.3
OUT = os.path.join(ROOT, "profiles", "depth_prune", "probe.jsonl")
os.makedirs(os.path.dirname(OUT), exist_ok=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def scene_mm(rng):
    """one depth image in millimetres (float64): ground plane, boxes, holes"""
    d = np.repeat(np.linspace(6000.0, 1000.0, ROWS)[:, None], COLS, axis=1)
    for _ in range(12):
        z = rng.uniform(800.0, 4500.0)
        w = int(FX * 600.0 / z)                       # a box 0.6 m wide, 1.5 times as tall
        x, y = int(rng.integers(0, COLS - 8)), int(rng.integers(0, ROWS - 8))
        sub = d[y:y + 3 * w // 2, x:x + w]
        sub[sub > z] = z                              # nearer surfaces hide farther ones
    d[rng.random((ROWS, COLS)) < 0.03] = 0.0
    return d


rng = np.random.default_rng(seed)
mm = np.stack([scene_mm(rng) for _ in range(B)])
depth = {"16U": (np.rint(mm).astype(np.uint16), 2, WIDTH_M * 1000.0), "32F": ((mm / 1000.0).astype(np.float32), 5, WIDTH_M)}

det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16)
det.distributeModel(synthetic_person_model())
hd = det.hd
d = torch.from_numpy(np.stack([synth.synthetic_frame(i + 1, ROWS, COLS, 3) for i in range(B)])).cuda()


def timed_window(fn, seconds):
    """calls of fn for at least `seconds`: (calls, wall ms per call); fn ends in the read-back, so every call is complete"""
    hd.check(hd.lib.pbd_synchronize(hd.h))
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        n += 1
        if n % 64 == 0:
            hd.check(hd.lib.pbd_profile_read(hd.h, 0, None, None))
        if time.perf_counter() - t0 >= seconds:
            break
    return n, (time.perf_counter() - t0) * 1e3 / n


for name, (arr, code, width) in depth.items():
    view = arr.view(np.int16) if arr.dtype == np.uint16 else arr
    d_depth = torch.from_numpy(view).cuda()
    torch.cuda.synchronize()
    es = arr.dtype.itemsize
    descs = [(d_depth[f].data_ptr(), ROWS, COLS, COLS * es) for f in range(B)]

    def step(on):
        if on:
            hd.bind_depth_device(descs, code)
        _, n = det.detect_batch_device(d.data_ptr(), B, ROWS, COLS, 3, raw=True)
        return int(n)

    hd.set_depth_prune(FX, width, TOL)                  # on for the whole run: without a binding nothing is pruned
    rec = {"probe": "cost", "depth": name, "workload": f"{B}x{COLS}x{ROWS}", "fx": FX, "width": width, "tol": TOL, "seed": seed,
           "window_s": window}
    for nms in (None, 0.1):
        tag = "nms0.1" if nms is not None else "raw"
        hd.set_nms(nms)
        out = {"candidates": {}, "k_depth_prune_ms_per_step": None, "k_argmin_ms_per_step": {}, "end_to_end_ms_per_step": {"off": [], "on": []}}
        for key, on in (("off", False), ("on", True)):  # warm both; the counts
            out["candidates"][key] = step(on)
        for rnd in range(3):                            # end to end, profiling off, alternating windows
            for key, on in (("off", False), ("on", True)):
                out["end_to_end_ms_per_step"][key].append(round(timed_window(lambda: step(on), window)[1], 3))
        for key, on in (("off", False), ("on", True)):  # kernel times: event pairs on every launch, a run of their own
            hd.profile(1)
            n, _ = timed_window(lambda: step(on), window)
            prof = hd.profile_read()
            hd.profile(0)
            out["k_argmin_ms_per_step"][key] = round(prof["k_argmin"][0] / n, 4)
            if on:
                out["k_depth_prune_ms_per_step"] = round(prof["k_depth_prune"][0] / n, 4)
        rec[tag] = out
    emit(rec)
    hd.set_nms(None)
hd.set_depth_prune(None)
hd.close()
