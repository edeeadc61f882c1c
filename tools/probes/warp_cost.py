"""Cost of the warped positives (pbd_warp_positives*): 1024 boxes spread over 16 synthetic 640x480 frames, a one-part model with
k = 5, sbin = 4 (28 x 28 patches), T = float and double.  Per case: the kernel time of one device-form call from
pbd_profile_read (k_warp, k_hog_hist, k_hog_feat, k_warp_emit; HIP events per launch, the median run of `REPS`), the wall time of
the device form (frames resident, call + synchronise) and of the host form (frames uploaded, examples read back), each the median
of `REPS` runs after a warm-up, and next to them the numpy yardstick (partsbaseddetector_amd/warp.py: the CPU oracle's resize and
HOG) on the same boxes on the host.  Prints one JSON line per case; with an argument, also writes them to that file.

    python tools/probes/warp_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth, warp  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

REPS = 7
NFRAMES, NBOXES, K, SBIN = 16, 1024, 5, 4
KERNELS = ["k_warp", "k_hog_hist", "k_hog_feat", "k_warp_emit"]


def boxes_of(rng):
    """boxes of 20..240 pixels a side, a tenth of them crossing a frame edge, none below the filter's 20 x 20 pixels"""
    b = np.zeros((NBOXES, 5), np.int32)
    b[:, 0] = np.arange(NBOXES) % NFRAMES
    w, h = rng.integers(20, 241, NBOXES), rng.integers(20, 241, NBOXES)
    b[:, 1] = rng.integers(-24, 640 - 20, NBOXES)
    b[:, 2] = rng.integers(-24, 480 - 20, NBOXES)
    b[:, 3] = b[:, 1] + w - 1
    b[:, 4] = b[:, 2] + h - 1
    return b


def median_wall(run, reps=REPS):
    run()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def main():
    import torch
    torch.cuda.init()
    frames = [synth.synthetic_frame(100 + s, 480, 640) for s in range(NFRAMES)]
    boxes = boxes_of(np.random.default_rng(3))
    model = M.synthetic_model(seed=5, pa=[0], nmix=1, ksize=K, sbin=SBIN, interval=5, name="one_part")
    flat = model.flatten()
    dev = [torch.from_numpy(f).cuda() for f in frames]
    descs = [(t.data_ptr(), 480, 640, 640 * 3) for t in dev]
    out = []
    for dtype in (np.float32, np.float64):
        real = _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64
        hd = detector.Handle(model, device=0, max_batch=NFRAMES, real_type=real)
        hw, vw = hd.example_stride()
        pay = torch.zeros(1 + NBOXES * hd.stride, dtype=torch.int32, device="cuda")
        d_hdr = torch.zeros(NBOXES * hw, dtype=torch.int32, device="cuda")
        d_val = torch.zeros(NBOXES * vw, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")

        def device_form():
            hd.warp_positives_device(descs, 3, 0, boxes, 0, 0, True, 0, pay.data_ptr(), NBOXES, d_hdr.data_ptr(), d_val.data_ptr())
            hd.check(hd.lib.pbd_synchronize(hd.h))

        def host_form():
            return hd.warp_positives(frames, boxes, 0, 0, True)

        device_wall = median_wall(device_form)
        host_wall = median_wall(host_form)
        runs = []
        for _ in range(REPS):
            hd.profile(True)
            device_form()
            prof = hd.profile_read()
            runs.append({k: prof[k][0] for k in KERNELS})
            hd.profile(False)
        runs.sort(key=lambda m: sum(m.values()))
        per = {k: round(v, 4) for k, v in runs[len(runs) // 2].items()}
        t0 = time.perf_counter()
        ref = warp.warp_examples(flat, frames, boxes, 0, 0, True, dtype)
        yard = round((time.perf_counter() - t0) * 1e3, 1)
        got = host_form()
        rec = {"case": f"{NBOXES} boxes, {NFRAMES} x 640x480, k={K}, sbin={SBIN}, T={np.dtype(dtype).name}", "kept": int(ref[2].sum()),
               "equal_to_yardstick": all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)),
               "kernel_ms": round(sum(per.values()), 4), "per_kernel_ms": per, "device_form_wall_ms": device_wall,
               "host_form_wall_ms": host_wall, "yardstick_host_ms": yard,
               "yardstick_over_device_form": round(yard / device_wall, 1), "yardstick_over_host_form": round(yard / host_wall, 1)}
        print(json.dumps(rec))
        out.append(rec)
        hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
