"""Cost of the 3-D box stage (pbd_boxes3d_device, k_boxes3d) on the two reference workloads: 64 x 640x480 and 8 x 1920x1080
frames, person model, synthetic_depth (16U, the colour frame's size), suppression at 0.1 -- and, for 640x480, with
suppression off (every candidate: the stress case).  Per workload the candidate list stays on the device
(pbd_detect_batch_device_out) and the stage runs `steps` times on it.  Run it under `rocprofv3 --kernel-trace --stats` and
read k_boxes3d from the kernel statistics (ms per step = its total / its calls); run it once more without the profiler for
the host figures.  Prints one JSON line per workload:
  M_min / M_median / M_max / M_total   samples per candidate (boxes counted with their overlaps), host-side count
  stage_ms_per_step                    wall clock of one stage call, synchronised, averaged over `steps`
  depth_bytes_read                     8 passes x M_total x 2 bytes: what the select reads through the caches per step
  mirror_ms / mirror_records           numpy mirror (Candidate.boundingBox3D) on the same records (a prefix of the list when
                                       it is long), for the caller's comparison

    python tools/probes/boxes3d_cost.py [steps] [mirror_records]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from partsbaseddetector_amd import synth  # noqa: E402
from partsbaseddetector_amd.detector import Candidate, PartsBasedDetector, _rect_and  # noqa: E402
from partsbaseddetector_amd.model import synthetic_person_model  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
mirror_cap = int(sys.argv[2]) if len(sys.argv) > 2 else 400


def samples(c: Candidate, rows, cols, depth):
    """M of one candidate: valid samples under its boxes, overlaps counted (the stage's pass-0 count)"""
    drows, dcols = depth.shape
    sx, sy = dcols / float(cols), drows / float(rows)
    boxes = [_rect_and(tuple(int(v) for v in r), (0, 0, cols, rows)) for r in c.parts]
    boxes.append(_rect_and(c.boundingBoxNorm(), (0, 0, cols, rows)))
    m = 0
    for x, y, w, h in boxes:
        x, y, w, h = _rect_and((int(x * sx), int(y * sy), int(w * sx), int(h * sy)), (0, 0, dcols, drows))
        if w > 0 and h > 0:
            m += int(np.count_nonzero(depth[y:y + h, x:x + w]))
    return m


model = synthetic_person_model()
for rows, cols, B, nms in ((480, 640, 64, 0.1), (480, 640, 64, None), (1080, 1920, 8, 0.1)):
    frames = np.stack([synth.synthetic_frame(i + 1, rows, cols, 3) for i in range(B)])
    depths = [synth.synthetic_depth(i + 1, rows, cols, np.uint16) for i in range(B)]
    d_frames = torch.from_numpy(frames).cuda()
    d_depth = torch.from_numpy(np.stack(depths).view(np.int16)).cuda()
    det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16, nms=nms)
    det.distributeModel(model)
    hd = det.hd
    cap = 1 << 16
    pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
    out = torch.zeros((cap, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, B, d_frames.data_ptr(), rows, cols, 3, 0, pay.data_ptr(), cap))
    hd.check(hd.lib.pbd_synchronize(hd.h))
    p = pay.cpu().numpy()
    n = int(p[0])
    rec = p[1:1 + n * hd.stride].reshape(n, hd.stride).copy()
    descs = [(d_depth[f].data_ptr(), rows, cols, cols * 2) for f in range(B)]
    shapes = [(rows, cols)] * B
    hd.boxes3d_device(descs, 2, shapes, pay.data_ptr(), cap, 0, out.data_ptr())     # warm-up
    hd.check(hd.lib.pbd_synchronize(hd.h))
    t0 = time.perf_counter()
    for _ in range(steps):
        hd.boxes3d_device(descs, 2, shapes, pay.data_ptr(), cap, 0, out.data_ptr())
    hd.check(hd.lib.pbd_synchronize(hd.h))
    stage_ms = (time.perf_counter() - t0) * 1e3 / steps
    got = out[:n].cpu().numpy()
    cands = hd.unpack_candidates(rec.ravel(), n)
    ms = np.array([samples(c, rows, cols, depths[c.frame]) for c in cands], np.int64)
    k = min(n, mirror_cap)
    t0 = time.perf_counter()
    want = np.array([c.boundingBox3D((rows, cols), depths[c.frame]) for c in cands[:k]]).reshape(-1, 6)
    mirror_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(got[:k].view(np.uint64), want.view(np.uint64)))
    print(json.dumps({
        "workload": f"{B}x{cols}x{rows}", "nms": nms, "candidates": n, "steps": steps,
        "M_min": int(ms.min()), "M_median": float(np.median(ms)), "M_max": int(ms.max()), "M_total": int(ms.sum()),
        "stage_ms_per_step": round(stage_ms, 3), "depth_bytes_read": int(8 * ms.sum() * 2),
        "mirror_ms": round(mirror_ms, 1), "mirror_records": k, "mirror_equal": same}), flush=True)
    hd.close()
