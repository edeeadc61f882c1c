"""Cost of the per-frame sort + non-maxima suppression stage (pbd_set_nms) on the two reference workloads: 64 x 640x480 and
8 x 1920x1080 frames, person model.  Each workload runs `steps` batches with the stage off, then `steps` with it on at
overlap 0.1; run it under `rocprofv3 --kernel-trace --stats` and read k_post_* from the kernel statistics (the added kernel
time per step = their total / steps).  Prints one JSON line per workload: candidates per step before / after suppression,
the bytes each read-back moves, and wall-clock ms per step off / on.

    python tools/probes/nms_cost.py [steps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from partsbaseddetector_amd import synth  # noqa: E402
from partsbaseddetector_amd.detector import PartsBasedDetector  # noqa: E402
from partsbaseddetector_amd.model import synthetic_person_model  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
model = synthetic_person_model()
for rows, cols, B in ((480, 640, 64), (1080, 1920, 8)):
    frames = np.stack([synth.synthetic_frame(i + 1, rows, cols, 3) for i in range(B)])
    d = torch.from_numpy(frames).cuda()
    det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16)
    det.distributeModel(model)
    out = {"workload": f"{B}x{cols}x{rows}", "steps": steps}
    for tag, ov in (("off", None), ("on", 0.1)):
        det.hd.set_nms(ov)
        _, n = det.detect_batch_device(d.data_ptr(), B, rows, cols, 3, raw=True)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            _, n = det.detect_batch_device(d.data_ptr(), B, rows, cols, 3, raw=True)
        out[f"ms_per_step_{tag}"] = round((time.perf_counter() - t0) * 1e3 / steps, 3)
        out[f"candidates_{tag}"] = int(n)
        out[f"readback_bytes_{tag}"] = 4 * (1 + int(n) * det.hd.stride)
    print(json.dumps(out), flush=True)
    det.hd.close()
