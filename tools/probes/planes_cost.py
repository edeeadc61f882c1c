"""Cost of plane removal (pbd_remove_planes_device: the k_pl_* kernels) on three workloads: one 640x480 room, one 1920x1080 room,
and a batch of 64 640x480 rooms in one call (tests/planes_scenes.py: floor, wall, two boxes, a ball, holes).  The clouds are on
the device; each step is one call, nothing read back.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(ms per step = a kernel's total / (steps + 1)).  Prints one JSON line per workload:
  planes / kept            planes of the first cloud, kept points of all clouds
  stage_ms_per_step        wall clock of the call, synchronised, averaged over `steps`
  mirror_ms_per_cloud      the numpy yardstick (PointCloudClusterer.organizedMultiplaneSegmentation) on one cloud
  mirror_equal             the device's labels, planes and reduced cloud of the first cloud equal the yardstick's

    python tools/probes/planes_cost.py [steps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import planes_scenes as S  # noqa: E402
from partsbaseddetector_amd.detector import Handle  # noqa: E402
from partsbaseddetector_amd.model import synthetic_tiny_model  # noqa: E402
from partsbaseddetector_amd.pointcloud import PointCloudClusterer as PCC  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
hd = Handle(synthetic_tiny_model(), device=0)
for rows, cols, B in ((480, 640, 1), (1080, 1920, 1), (480, 640, 64)):
    room, _ = S.room(rows, cols)
    n = rows * cols
    d_cloud = torch.from_numpy(np.ascontiguousarray(room)).cuda()
    descs = [(d_cloud.data_ptr(), rows, cols, 12, cols * 12)] * B
    pts = torch.zeros((B * n, 3), dtype=torch.float32, device="cuda")
    kept = torch.zeros(B * n, dtype=torch.int32, device="cuda")
    lab = torch.zeros(B * n, dtype=torch.int32, device="cuda")
    nk = torch.zeros(B, dtype=torch.int32, device="cuda")
    npl = torch.zeros(B, dtype=torch.int32, device="cuda")
    cap = 16
    pl = torch.zeros((B * cap, 4), dtype=torch.float32, device="cuda")
    inl = torch.zeros(B * cap, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")

    def step():
        hd.remove_planes_device(descs, None, pts.data_ptr(), kept.data_ptr(), nk.data_ptr(), lab.data_ptr(), pl.data_ptr(),
                                inl.data_ptr(), npl.data_ptr(), cap, st.data_ptr())

    step()
    hd.check(hd.lib.pbd_synchronize(hd.h))
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    hd.check(hd.lib.pbd_synchronize(hd.h))
    stage_ms = (time.perf_counter() - t0) * 1e3 / steps
    t0 = time.perf_counter()
    wp, wk, wl, wpl = PCC.organizedMultiplaneSegmentation(room)
    mirror_ms = (time.perf_counter() - t0) * 1e3
    k0 = int(nk[0].item())
    same = bool(np.array_equal(lab[:n].cpu().numpy().reshape(rows, cols), wl) and int(npl[0].item()) == len(wpl) and
                np.array_equal(pl[:len(wpl)].cpu().numpy().view(np.uint32), wpl.view(np.uint32)) and
                np.array_equal(pts[:k0].cpu().numpy().view(np.uint32), wp.view(np.uint32)) and
                np.array_equal(kept[:k0].cpu().numpy(), wk))
    print(json.dumps({"workload": f"{B}x{cols}x{rows}", "steps": steps, "planes": int(npl[0].item()), "kept": int(st[0].item()),
                      "stage_ms_per_step": round(stage_ms, 3), "mirror_ms_per_cloud": round(mirror_ms, 1),
                      "mirror_equal": same}), flush=True)
hd.close()
