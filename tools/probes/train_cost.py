"""Cost of one train() iteration and of the two walks (pbd_set_walk) on one MI355X.  Person model (26 parts x 6 mixtures),
64 negatives of 640 x 480, 16 latent positives of 240 x 320, a cache of 10 000 examples, negatives mined 8 frames at a time.

  stages   wall clock of every device call train() makes, summed per stage; every asynchronous call is followed by a
           synchronisation here so that its time is its own (train() itself does not wait there)
  walks    k_argmin (find + walk of a 64 x 640 x 480 step) and k_ex_walk (131 072 records) in both modes, alternating in one
           process, HIP events per launch, 7 repetitions each: median, minimum and maximum

Prints one JSON line per measurement; with an argument, also writes them to that file.

    python tools/probes/train_cost.py [out.jsonl]
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
from partsbaseddetector_amd import train as T  # noqa: E402


def positives(model, n):
    """n frames with the part boxes of the model's own best placement (any score) whose every part has at least minsize pixels"""
    det = detector.PartsBasedDetector(device=0, max_candidates=1 << 20)
    det.setWalk("argmax")
    low = M.synthetic_person_model(thresh=-1000.0)
    det.distributeModel(low)
    pos = []
    for s in range(n):
        im = synth.synthetic_frame(100 + s, 240, 320)
        ok = [c for c in det.detect(im) if all((w + 1) * (h + 1) >= 400 for _, _, w, h in c.parts)]
        best = max(ok, key=lambda c: c.score())
        pos.append({"im": im, "boxes": np.array([(x, y, x + w, y + h) for x, y, w, h in best.parts], np.int32)})
    det.hd.close()
    return pos


def timed(stages, name, fn, sync):
    def wrapper(*a, **k):
        sync()
        t = time.perf_counter()
        out = fn(*a, **k)
        sync()
        stages[name] = stages.get(name, 0.0) + (time.perf_counter() - t) * 1e3
        stages[name + "_calls"] = stages.get(name + "_calls", 0) + 1
        return out
    return wrapper


def stage_times(model, pos, neg):
    import torch
    stages = {}
    sync = torch.cuda.synchronize
    P, QP = detector.PartsBasedDetector, Q.QP
    saved = [(P, n, getattr(P, n)) for n in ("detect_frames_device_out", "examples_device", "updateModel")] + \
            [(QP, n, getattr(QP, n)) for n in ("add_device", "add_loss_device", "opt", "one", "prune")] + [(T, "_detect_latent", T._detect_latent)]
    names = {"detect_frames_device_out": "mine_detect", "examples_device": "examples", "updateModel": "update", "add_device": "add_device",
             "add_loss_device": "add_loss", "opt": "passes_opt", "one": "passes_one", "prune": "prune", "_detect_latent": "latent_search"}
    for owner, n, fn in saved:
        setattr(owner, n, timed(stages, names[n], fn, sync))
    try:
        t = time.perf_counter()
        _, info = T.train(model, pos, neg, 0, capacity=10000, neg_batch=8, max_passes=10)
        total = (time.perf_counter() - t) * 1e3
    finally:
        for owner, n, fn in saved:
            setattr(owner, n, fn)
    return {"case": "one iteration: person model, 16 latent positives 240x320, 64 negatives 640x480, cache 10000, neg_batch 8, max_passes 10",
            "total_ms": round(total, 1), "stages_ms": {k: (round(v, 2) if isinstance(v, float) else v) for k, v in sorted(stages.items())},
            "numpositives": info["numpositives"], "branches": [b["branch"] for b in info["batches"]],
            "found": [b["found"] for b in info["batches"]], "taken": [b["taken"] for b in info["batches"]],
            "n": info["n"], "nsv": info["nsv"], "lb": info["lb"], "ub": info["ub"]}


def walk_times(reps=7):
    import torch
    model = M.synthetic_person_model(thresh=M.PERSON_THRESH - 1.0)
    hd = detector.Handle(model, device=0, max_batch=64, max_candidates=1 << 17)
    d_frames = torch.from_numpy(np.stack([synth.synthetic_frame(s, 480, 640) for s in range(64)])).cuda()
    cap = 1 << 17
    pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
    hw, vw = hd.example_stride()
    d_hdr = torch.empty((cap, hw), dtype=torch.int32, device="cuda")
    d_val = torch.empty((cap, vw), dtype=torch.float32, device="cuda")
    hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, 64, d_frames.data_ptr(), 480, 640, 3, 0, pay.data_ptr(), cap))
    hd.check(hd.lib.pbd_synchronize(hd.h))
    n = min(int(pay[0].item()), cap)
    ms = {("reference", "k_argmin"): [], ("reference", "k_ex_walk"): [], ("argmax", "k_argmin"): [], ("argmax", "k_ex_walk"): []}
    for _ in range(reps):
        for name, mode in (("reference", _lib.WALK_REFERENCE), ("argmax", _lib.WALK_ARGMAX)):
            hd.set_walk(mode)
            hd.profile(True)
            hd.check(hd.lib.pbd_argmin_device_out(hd.h, 0, pay.data_ptr(), cap))
            hd.examples_device(pay.data_ptr(), n, 0, d_hdr.data_ptr(), d_val.data_ptr())
            hd.check(hd.lib.pbd_synchronize(hd.h))
            prof = hd.profile_read()
            hd.profile(False)
            for k in ("k_argmin", "k_ex_walk"):
                ms[(name, k)].append(prof[k][0])
    hd.close()
    out = {"case": "64 x 640x480, person model, 131072 records walked: HIP-event ms per launch, alternating modes", "records": n}
    for (name, k), v in ms.items():
        v = sorted(v)
        out[f"{k}_{name}"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    return out


def main():
    import torch
    torch.cuda.init()
    out = [walk_times()]
    print(json.dumps(out[-1]), flush=True)
    model = M.synthetic_person_model()
    pos = positives(model, 16)
    neg = [synth.synthetic_frame(s, 480, 640) for s in range(64)]
    out.append(stage_times(model, pos, neg))
    print(json.dumps(out[-1]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
