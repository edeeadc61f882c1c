"""Cost of the camera-box and clustering stages (pbd_boxes3d_camera_device: k_boxes3d + k_camera_boxes; pbd_cluster_objects_device:
the k_cl_* kernels) on three workloads: 64 x 640x480 with suppression at 0.1 and off, 8 x 1920x1080 at 0.1.  Person model,
synthetic_depth(i + 1, float32 metres) per frame, one camera (fx = fy = 525, the image centre), clouds from cloud_from_depth on
the device.  The candidate list stays on the device (pbd_detect_batch_device_out); each step is one camera call and one
clustering call on it, nothing read back.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (ms per
step = a kernel's total / steps + 1).  Prints one JSON line per workload:
  crop_min / _median / _max / _total   points cropped per box (the yardstick's crop of the device's camera boxes)
  kept_total                           output indices (status[1])
  edge_candidates                      pairs j < i in the 27 neighbouring 2 cm cells over every box (what the grid hands the exact
                                       predicate, before hash collisions)
  stage_ms_per_step                    wall clock of both calls, synchronised, averaged over `steps`
  mirror_ms / mirror_boxes             the numpy yardstick (PointCloudClusterer.clusterObjects) on the first `mirror_boxes` boxes
                                       (0, the default: every box)
  mirror_equal                         the device's centres and indices equal the yardstick's on those boxes

    python tools/probes/pointcloud_cost.py [steps] [mirror_boxes]"""
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
from partsbaseddetector_amd.pointcloud import PinholeCamera, PointCloudClusterer as PCC, cloud_from_depth  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
mirror_cap = int(sys.argv[2]) if len(sys.argv) > 2 else 0

model = synthetic_person_model()
for rows, cols, B, nms in ((480, 640, 64, 0.1), (480, 640, 64, None), (1080, 1920, 8, 0.1)):
    cam = PinholeCamera(525.0, 525.0, (cols - 1) / 2.0, (rows - 1) / 2.0)
    frames = np.stack([synth.synthetic_frame(i + 1, rows, cols, 3) for i in range(B)])
    depths = [synth.synthetic_depth(i + 1, rows, cols, np.float32) for i in range(B)]
    clouds = [cloud_from_depth(d, cam) for d in depths]
    d_frames = torch.from_numpy(frames).cuda()
    d_depth = torch.from_numpy(np.stack(depths)).cuda()
    d_cloud = torch.from_numpy(np.stack(clouds)).cuda()
    det = PartsBasedDetector(device=0, max_batch=B, max_candidates=1 << 16, nms=nms)
    det.distributeModel(model)
    hd = det.hd
    cap = 1 << 14
    pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
    box = torch.zeros((cap, 6), dtype=torch.float64, device="cuda")
    cen = torch.zeros((cap, hd.max_parts, 3), dtype=torch.float32, device="cuda")
    nc = torch.zeros(cap, dtype=torch.int32, device="cuda")
    dn = torch.zeros(cap, dtype=torch.int32, device="cuda")
    oc = torch.zeros((cap, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(cap, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, B, d_frames.data_ptr(), rows, cols, 3, 0, pay.data_ptr(), cap))
    descs = [(d_depth[f].data_ptr(), rows, cols, cols * 4) for f in range(B)]
    cdescs = [(d_cloud[f].data_ptr(), rows, cols, 12, cols * 12) for f in range(B)]
    shapes, cams = [(rows, cols)] * B, [cam] * B
    crop_cap = min(B * rows * cols, (1 << 30) - 1)
    idx = torch.zeros(crop_cap, dtype=torch.int32, device="cuda")

    def step(crop_cap):
        hd.boxes3d_camera_device(descs, 5, shapes, cams, 0, pay.data_ptr(), cap, 0, box.data_ptr(), cen.data_ptr(), nc.data_ptr(),
                                 dn.data_ptr())
        hd.cluster_objects_device(cdescs, pay.data_ptr(), cap, 0, box.data_ptr(), crop_cap, idx.numel(), oc.data_ptr(),
                                  cnt.data_ptr(), idx.data_ptr(), st.data_ptr())

    step(crop_cap)                                  # warm-up, and the cropped total for the workspace of the timed steps
    hd.check(hd.lib.pbd_synchronize(hd.h))
    crop_cap = int(st[0].item())
    if crop_cap >= 1 << 30:
        print(json.dumps({"workload": f"{B}x{cols}x{rows}", "nms": nms, "device_crop_total": crop_cap, "skipped": "over 2^30 points"}))
        hd.close()
        continue
    idx = torch.zeros(max(crop_cap, 1), dtype=torch.int32, device="cuda")
    t0 = time.perf_counter()
    for _ in range(steps):
        step(crop_cap)
    hd.check(hd.lib.pbd_synchronize(hd.h))
    stage_ms = (time.perf_counter() - t0) * 1e3 / steps
    p = pay.cpu().numpy()
    n = int(p[0])
    rec = p[1:1 + n * hd.stride].reshape(n, hd.stride)
    bx = box[:n].cpu().numpy()
    s = st.cpu().numpy()
    print(f"{B}x{cols}x{rows} nms {nms}: {n} boxes, {stage_ms:.3f} ms per step; host-side counts follow", file=sys.stderr, flush=True)
    crops = np.array([len(PCC.crop(clouds[int(rec[i, 0])], bx[i])) for i in range(n)], np.int64)
    k = min(n, mirror_cap) if mirror_cap > 0 else n
    t0 = time.perf_counter()
    wc, wi = np.zeros((0, 3), np.float32), []
    for b0 in range(0, k, 50):                      # in blocks, with a progress line each
        c_, i_ = PCC.clusterObjects(clouds, bx[b0:min(b0 + 50, k)], rec[b0:min(b0 + 50, k), 0])
        wc, wi = np.concatenate([wc, c_]), wi + i_
        print(f"  yardstick {min(b0 + 50, k)} / {k}", file=sys.stderr, flush=True)
    mirror_ms = (time.perf_counter() - t0) * 1e3
    edges = sum(PCC.edgeCandidates(clouds[int(rec[i, 0])].reshape(-1, 3)[PCC.crop(clouds[int(rec[i, 0])], bx[i])]) for i in range(n))
    c = cnt[:n].cpu().numpy()
    off = np.concatenate([[0], np.cumsum(c)])
    ix = idx[:int(off[k])].cpu().numpy()
    same = bool(np.array_equal(oc[:k].cpu().numpy().view(np.uint32), wc.view(np.uint32)) and
                all(np.array_equal(ix[off[i]:off[i + 1]], wi[i]) for i in range(k)))
    print(json.dumps({
        "workload": f"{B}x{cols}x{rows}", "nms": nms, "boxes": n, "steps": steps,
        "crop_min": int(crops.min()), "crop_median": float(np.median(crops)), "crop_max": int(crops.max()),
        "crop_total": int(crops.sum()), "device_crop_total": int(s[0]), "kept_total": int(s[1]),
        "edge_candidates": int(edges), "stage_ms_per_step": round(stage_ms, 3),
        "mirror_ms": round(mirror_ms, 1), "mirror_boxes": k, "mirror_equal": same}), flush=True)
    hd.close()
