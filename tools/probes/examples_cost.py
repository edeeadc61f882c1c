"""Kernel time of the training examples (pbd_examples_device: k_ex_walk + k_ex_gather) on every record of a 64 x 640x480 step of
the synthetic person model at a low threshold, in ms and in GB/s of the bytes the gather must move (each example's values and
header written, its feature windows read), against the step's detect time.  Prints one JSON line per case; with an argument, also
writes them to that file.

    python tools/probes/examples_cost.py [out.jsonl]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402


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
    return round(sum(best.values()), 4), {k: round(v, 4) for k, v in best.items()}


def main():
    import torch
    torch.cuda.init()
    out = []
    for thresh, dtype in ((M.PERSON_THRESH - 1.0, np.float32), (M.PERSON_THRESH - 1.0, np.float64)):
        model = M.synthetic_person_model(thresh=thresh)
        real = _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64
        hd = detector.Handle(model, device=0, max_batch=64, max_candidates=1 << 17, real_type=real)
        frames = np.stack([synth.synthetic_frame(s, 480, 640) for s in range(64)])
        d_frames = torch.from_numpy(frames).cuda()
        cap = 1 << 17
        pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")

        def detect():
            hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, 64, d_frames.data_ptr(), 480, 640, 3, 0, pay.data_ptr(), cap))

        det_ms, _ = kernel_ms(hd, [k for k in _lib.KERNELS if not k.startswith(("k_ex", "k_cl", "k_dc", "k_mk", "k_part", "k_camera"))],
                              detect)
        detect()
        hd.check(hd.lib.pbd_synchronize(hd.h))
        found = int(pay[0].item())
        n = min(found, cap)     # the first `cap` records of the step when more were found
        assert n > 0
        hw, vw = hd.example_stride()
        d_hdr = torch.empty((n, hw), dtype=torch.int32, device="cuda")
        d_val = torch.empty((n, vw), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
        ex_ms, per = kernel_ms(hd, ["k_ex_walk", "k_ex_gather"],
                               lambda: hd.examples_device(pay.data_ptr(), n, 0, d_hdr.data_ptr(), d_val.data_ptr()))
        hd.check(hd.lib.pbd_synchronize(hd.h))
        nv = d_hdr[:, 3].to(torch.int64)
        vbytes = int(nv.sum().item()) * np.dtype(dtype).itemsize
        moved = 2 * vbytes + n * hw * 4   # windows read + values written + headers written
        rec = {"case": f"64 x 640x480, person model, thresh {thresh:.2f}, T={np.dtype(dtype).name}", "found": found, "examples": n,
               "values_per_example": round(float(nv.float().mean().item()), 1), "bytes_per_example": round(vbytes / n),
               "examples_ms": ex_ms, "per_kernel_ms": per, "gather_GBps": round(moved / (per["k_ex_gather"] * 1e-3) / 1e9, 1),
               "all_GBps": round(moved / (ex_ms * 1e-3) / 1e9, 1), "detect_kernels_ms": det_ms}
        print(json.dumps(rec))
        out.append(rec)
        hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
