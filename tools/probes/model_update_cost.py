"""What giving a handle new weights costs, three ways, through to the first completed detect of one 640x480 frame:

  device   pbd_set_model_vector_device from a vector already on the device
  apply    pbd_qp_apply from a training QP
  create   the way before the in-place update: pbd_qp_weights, Model.from_vector, destroy + pbd_create

for the person model in PBD_CONV_EXACT float, PBD_CONV_MFMA and PBD_CONV_MFMA_F64.  One process; the three ways alternate
inside every repetition so that clock and cache state are shared; two warm-up repetitions, then the median (and the spread)
of --reps.  Wall-clock times of the calling thread: every call here ends synchronised (the update reads its status block
back, detect returns its records).  Prints one JSON line per mode.

    timeout -k 10 600 python tools/probes/model_update_cost.py --out profiles/model_update/probe.jsonl
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/probes/model_update_cost.py --trace-one
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402
from partsbaseddetector_amd import qp as Q  # noqa: E402

MODES = [("exact_f32", np.float32, _lib.CONV_EXACT), ("mfma_bf16", np.float32, _lib.CONV_MFMA), ("mfma_f64", np.float64, _lib.CONV_MFMA_F64)]


def detect(hd, im, buf):
    n = C.c_int()
    hd.check(hd.lib.pbd_detect(hd.h, im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], im.strides[0], buf.ctypes.data,
                               hd.max_candidates, C.byref(n)))
    return n.value


def make_handle(model, dtype, mode):
    return detector.Handle(model, device=0, real_type=_lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64, conv_mode=mode,
                           max_candidates=1 << 16)


def trained_qp(hd, im, buf):
    """a QP holding a few examples of one detect, after a few passes: weights that are a model"""
    n = detect(hd, im, buf)
    rec = buf[: n * hd.stride].reshape(n, hd.stride)[:48].copy()
    hdr, vals = hd.examples(rec)
    q = Q.QP(hd, 64)
    q.add(hd, hdr[:12], vals[:12], rec[:12], label=1)
    q.fix()
    q.add(hd, hdr[12:], vals[12:], rec[12:], label=-1)
    q.opt(tol=0.05, iter=3, seed=1)
    return q


def median_ms(xs):
    xs = sorted(xs)
    return {"median_ms": round(1e3 * xs[len(xs) // 2], 3), "min_ms": round(1e3 * xs[0], 3), "max_ms": round(1e3 * xs[-1], 3)}


def run_mode(name, dtype, mode, reps, warm, trace_one):
    import torch
    model = M.synthetic_person_model()
    im = synth.synthetic_frame(1, 480, 640)
    hd = make_handle(model, dtype, mode)
    buf = np.zeros(hd.max_candidates * hd.stride, np.int32)
    q = trained_qp(hd, im, buf)
    w = q.weights()
    d_w = torch.from_numpy(w).cuda()
    torch.cuda.synchronize()
    if trace_one:
        hd.set_model_vector_device(d_w.data_ptr(), np.float64)
        detect(hd, im, buf)
        return {"mode": name, "traced": "one pbd_set_model_vector_device and one detect"}
    other = make_handle(model, dtype, mode)
    t = {k: [] for k in ("device_update", "device_total", "apply_update", "apply_total", "create_build", "create_total")}
    for r in range(warm + reps):
        a = time.perf_counter()
        hd.set_model_vector_device(d_w.data_ptr(), np.float64)
        b = time.perf_counter()
        detect(hd, im, buf)
        c = time.perf_counter()
        q.apply(hd)
        d = time.perf_counter()
        detect(hd, im, buf)
        e = time.perf_counter()
        new_model = model.from_vector(q.weights().astype(dtype))
        other.close()
        other = make_handle(new_model, dtype, mode)
        f = time.perf_counter()
        detect(other, im, buf)
        g = time.perf_counter()
        if r >= warm:
            for k, v in (("device_update", b - a), ("device_total", c - a), ("apply_update", d - c), ("apply_total", e - c),
                         ("create_build", f - e), ("create_total", g - e)):
                t[k].append(v)
    same = other.model_vector().tobytes() == hd.model_vector().tobytes()
    out = {"mode": name, "frame": [480, 640], "reps": reps, "warmup": warm, "vectors_equal": bool(same)}
    out.update({k: median_ms(v) for k, v in t.items()})
    hd.close(); other.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-one", action="store_true", help="one update and one detect in PBD_CONV_EXACT float, for a kernel trace")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    lines = []
    for name, dtype, mode in MODES[:1] if args.trace_one else MODES:
        res = run_mode(name, dtype, mode, args.reps, args.warmup, args.trace_one)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
