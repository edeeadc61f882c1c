"""Kernel time of the depth-consistency filter (pbd_depth_consistency) on the unsuppressed candidate list of a whole step, with the
total sample count it reads: 64 x 640x480 and 8 x 1920x1080 frames of the synthetic person model, both real types, a 32F depth
image per frame.  Prints one JSON line per case; with an argument, also writes them to that file.

    python tools/probes/depth_consistency_cost.py [out.jsonl]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402


def raw_batch(hd, frames):
    fr = [np.ascontiguousarray(f) for f in frames]
    rows, cols, cn = fr[0].shape
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    n = C.c_int()
    hd.check(hd.lib.pbd_detect_batch(hd.h, len(fr), _lib.ptr_array(fr), rows, cols, cn, cols * cn, buf.ctypes.data,
                                     hd.max_candidates, C.byref(n)))
    return buf[: n.value * hd.stride].reshape(n.value, hd.stride).copy()


def samples(rec, rows, cols):
    """the clipped part areas of every (record, part) the filter reads (records of one-part components read none)"""
    np_ = rec[:, 6]
    total = 0
    for j in range(int(np_.max())):
        x, y, w, h = (rec[:, 8 + 4 * j + k].astype(np.int64) for k in range(4))
        x1, y1 = np.maximum(x, 0), np.maximum(y, 0)
        x2, y2 = np.minimum(x + w, cols), np.minimum(y + h, rows)
        a = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
        total += int(a[(np_ > j) & (np_ > 1)].sum())
    return total


def main():
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model()
    out = []
    for nf, rows, cols in ((64, 480, 640), (8, 1080, 1920)):
        frames = [synth.synthetic_frame(s, rows, cols) for s in range(nf)]
        depths = [synth.synthetic_depth(100 + s, rows, cols, np.float32) for s in range(nf)]
        for rt in (_lib.REAL_F32, _lib.REAL_F64):
            hd = detector.Handle(model, device=0, max_batch=nf, real_type=rt)
            rec = raw_batch(hd, frames)
            ms = []
            for _ in range(5):
                hd.profile(True)
                t0 = time.perf_counter()
                kept = hd.depth_consistency(depths, rec, 0.03)
                wall = time.perf_counter() - t0
                prof = hd.profile_read()
                ms.append((sum(prof[k][0] for k in ("k_dc_classify", "k_dc_select", "k_dc_compact")),
                           {k: round(prof[k][0], 4) for k in ("k_dc_classify", "k_dc_select", "k_dc_compact")}, wall * 1e3))
                hd.profile(False)
            best = sorted(ms, key=lambda m: m[0])[len(ms) // 2]
            row = {"frames": nf, "rows": rows, "cols": cols, "real": "f32" if rt == _lib.REAL_F32 else "f64", "records": len(rec),
                   "kept": len(kept), "samples": samples(rec, rows, cols), "kernel_ms_median": round(best[0], 4),
                   "kernel_ms_all": [round(m[0], 4) for m in ms], "per_kernel_ms": best[1], "call_wall_ms": round(best[2], 2)}
            print(json.dumps(row), flush=True)
            out.append(row)
            hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for row in out:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
