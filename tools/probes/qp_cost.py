"""Cost of the training QP (pbd_qp_*) on caches of 10 000 and 100 000 person-model examples mined from one 64 x 640x480 step
(every record at PERSON_THRESH - 1; the first 10 % are added as positives and fixed, the rest as negatives): wall time of
add_device, of a coordinate pass (pbd_qp_one: the k_qp_pass kernel plus the host's grouping and the refresh), of the whole-cache
score (pbd_qp_scores path) and of prune.  Prints one JSON line per cache size; with an argument, also writes them to that file.
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (profiles/qp/README.md).

    python tools/probes/qp_cost.py [out.jsonl] [--sizes 10000,100000]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402
from partsbaseddetector_amd import qp as Q  # noqa: E402


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    import torch
    torch.cuda.init()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sizes = [10000, 100000]
    for a in sys.argv[1:]:
        if a.startswith("--sizes="):
            sizes = [int(s) for s in a.split("=", 1)[1].split(",")]
    model = M.synthetic_person_model(thresh=M.PERSON_THRESH - 1.0)
    hd = detector.Handle(model, device=0, max_batch=64, max_candidates=1 << 17)
    frames = np.stack([synth.synthetic_frame(s, 480, 640) for s in range(64)])
    d_frames = torch.from_numpy(frames).cuda()
    cap = 1 << 17
    pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
    hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, 64, d_frames.data_ptr(), 480, 640, 3, 0, pay.data_ptr(), cap))
    torch.cuda.synchronize()
    found = int(pay[0].item())
    hw, vw = hd.example_stride()
    out = []
    for N in sizes:
        N = min(N, found, cap)
        P = N // 10
        q = Q.QP(hd, N)
        d_hdr = torch.empty((N - P, hw), dtype=torch.int32, device="cuda")
        d_val = torch.empty((N - P, vw), dtype=torch.float32, device="cuda")
        add_ms = 0.0
        for lo, hi, label, base in ((0, P, 1, 0), (P, N, -1, 1000)):
            sub = torch.empty(1 + (hi - lo) * hd.stride, dtype=torch.int32, device="cuda")
            sub[0] = hi - lo
            sub[1:] = pay[1 + lo * hd.stride:1 + hi * hd.stride]
            hd.examples_device(sub.data_ptr(), hi - lo, 0, d_hdr.data_ptr(), d_val.data_ptr())
            ms, _ = wall(lambda: q.add_device(hd, sub.data_ptr(), hi - lo, d_hdr.data_ptr(), d_val.data_ptr(), label, base))
            add_ms += ms
            if label == 1:
                q.fix()
        del d_hdr, d_val
        st = q.state()
        passes = []
        for t in range(3):
            nsv = q.state()["nsv"]
            ms, s = wall(lambda: q.one(seed=t))
            passes.append({"nsv": nsv, "ms": round(ms, 2), "us_per_step": round(ms * 1e3 / nsv, 3), "lb": s["lb"], "ub": s["ub"]})
        score_ms, _ = wall(q.scores)
        prune_ms, n1 = wall(q.prune)
        ms_opt, so = wall(lambda: q.opt(tol=0.05, iter=20, seed=100))
        rec = {"n": st["n"], "positives": P, "values": vw, "bytes_per_entry": vw * 5 + 8 * 3 + 1 + 4 * (st["hdr_words"] + 5),
               "add_device_ms": round(add_ms, 2), "passes": passes, "scores_ms": round(score_ms, 2), "prune_ms": round(prune_ms, 2),
               "after_prune": n1, "opt_ms": round(ms_opt, 1), "opt": {k: so[k] for k in ("passes", "converged", "lb", "ub", "nsv")}}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        q.close()
        torch.cuda.empty_cache()
    if args:
        with open(args[0], "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
