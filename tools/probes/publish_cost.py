"""Kernel time of the candidate mask (pbd_candidate_mask_device: labels plus the in-place masking of 3-channel frames) and of the
part-centre poses (pbd_part_poses_device) against the numpy yardsticks' host time (publish.frame_masks + masked_image,
publish.part_poses): the synthetic person model's kept (overlap 0.1) and unsuppressed lists of a 64 x 640x480 step and of an
8 x 1920x1080 step.  Prints one JSON line per case; with an argument, also writes them to that file.

    python tools/probes/publish_cost.py [out.jsonl]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, publish, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402
from partsbaseddetector_amd.pointcloud import PinholeCamera  # noqa: E402


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def kernel_ms(hd, names, run, reps=5):
    ms = []
    for _ in range(reps):
        hd.profile(True)
        run()
        hd.check(hd.lib.pbd_synchronize(hd.h))
        prof = hd.profile_read()
        ms.append({k: prof[k][0] for k in names})
        hd.profile(False)
    ms.sort(key=lambda m: sum(m.values()))
    best = ms[len(ms) // 2]
    return round(sum(best.values()), 4), {k: round(v, 4) for k, v in best.items()}, [round(sum(m.values()), 4) for m in ms]


def main():
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model()
    cam = PinholeCamera(525.0, 525.0, 319.5, 239.5)
    out = []
    for nf, rows, cols in ((64, 480, 640), (8, 1080, 1920)):
        frames = [synth.synthetic_frame(s, rows, cols) for s in range(nf)]
        depths = [synth.synthetic_depth(100 + s, rows, cols, np.float32) for s in range(nf)]
        hd = detector.Handle(model, device=0, max_batch=nf)
        raw = raw_batch(hd, frames)
        kept = hd.suppress([(rows, cols)] * nf, 0.1, raw)
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        d_labels = torch.zeros((nf, rows, cols), dtype=torch.uint8, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        for name, rec in (("kept", kept), ("unsuppressed", raw)):
            n = len(rec)
            pay = torch.from_numpy(np.concatenate([[n], rec.ravel()]).astype(np.int32)).cuda()
            ldesc = [(d_labels[f].data_ptr(), cols) for f in range(nf)]
            fdesc = [(d_frames[f].data_ptr(), cols * 3) for f in range(nf)]
            torch.cuda.synchronize()
            mk = kernel_ms(hd, ("k_mk_hull", "k_mk_tile"), lambda: hd.candidate_mask_device([(rows, cols)] * nf, pay.data_ptr(), n, 0,
                                                                                          ldesc, 3, fdesc, fdesc, st.data_ptr()))
            t0 = time.perf_counter()
            want = publish.frame_masks([(rows, cols)] * nf, rec)
            for f in range(nf):
                publish.masked_image(frames[f], want[f])
            host_mask_ms = (time.perf_counter() - t0) * 1e3
            assert int(st[0].item()) == n
            assert all(np.array_equal(d_labels[f].cpu().numpy(), want[f]) for f in range(nf))
            _, cen, nc, dn = hd.boxes3d_camera(depths, [(rows, cols)] * nf, [cam] * nf, rec)
            d_cen, d_nc, d_dn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cen, nc, dn))
            o_cnt = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
            o_pos, o_ori, o_ev = (torch.zeros((max(n, 1), k), dtype=torch.float32, device="cuda") for k in (3, 4, 3))
            torch.cuda.synchronize()
            ps = kernel_ms(hd, ("k_part_poses",), lambda: hd.part_poses_device(pay.data_ptr(), n, d_cen.data_ptr(), d_nc.data_ptr(),
                                                                               d_dn.data_ptr(), o_cnt.data_ptr(), o_pos.data_ptr(),
                                                                               o_ori.data_ptr(), o_ev.data_ptr()))
            t0 = time.perf_counter()
            publish.part_poses(cen, nc, dn)
            host_pose_ms = (time.perf_counter() - t0) * 1e3
            labelled = sum(int((w != 0).sum()) for w in want)
            row = {"frames": nf, "rows": rows, "cols": cols, "list": name, "records": n, "labelled_pixels": labelled,
                   "bytes_moved": nf * rows * cols * 7, "mask_kernel_ms_median": mk[0], "mask_per_kernel_ms": mk[1],
                   "mask_kernel_ms_all": mk[2], "mask_numpy_ms": round(host_mask_ms, 1), "pose_kernel_ms_median": ps[0],
                   "pose_kernel_ms_all": ps[2], "pose_numpy_ms": round(host_pose_ms, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
        hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for row in out:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
