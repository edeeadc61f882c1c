"""Cost of the augmented positives (pbd_augment_frames_device): 100 synthetic 640x480x3 8-bit frames, 10
copies of each -- mirror off and on x degrees (0, 7.5, -7.5, 15, -15) -- in ONE call of 1000 jobs.

Prints one JSON line: the device time of the call from a pair of HIP events on the handle's stream around it (the staged job and
tile tables' copy, 2.4 MB here, and k_augment, which has no id in the handle's profile; the median of `REPS` runs), the bytes the
call moves (every destination byte written once, every source pixel read once per job) and the fraction of
the HBM rate they amount to at that time (8 TB/s nominal, the figure DESIGN.md section 5 divides by, and the 6.29 TB/s measured
rate); the wall time of the call with the frames resident (call + synchronise, median of `REPS` after a warm-up); and the numpy
yardstick (augment.augment_positives_ref) on the host for the first `REF_FRAMES` frames, scaled to all of them.  With
`--latent`, a second line: the latent pass of one train() iteration over the positives of tests/train_cases.py's latent case
repeated `LATENT_COPIES` times, device-resident (pbd_detect_latent_device) against host frames (pbd_detect_latent), median wall
time of `REPS` runs each, alternating.  With a file argument the lines are also written there.

    python tools/probes/augment_cost.py [--latent] [out.jsonl]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import augment as A  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

REPS = 7
NFRAMES, REF_FRAMES = 100, 4
DEGREES = (7.5, -7.5, 15.0, -15.0)
HBM_NOMINAL, HBM_MEASURED = 8.0e12, 6.29e12
LATENT_COPIES = 8


def median_wall(run, reps=REPS):
    run()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def augment_line():
    import torch
    frames = [synth.synthetic_frame(100 + s, 480, 640) for s in range(NFRAMES)]
    cps = A.copies(DEGREES, [0])
    jobs = [(f, m, d) for f in range(NFRAMES) for m, d in cps]
    hd = detector.Handle(M.synthetic_tiny_model(), device=0)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    descs = [(t.data_ptr(), 480, 640, 640 * 3) for t in dev]
    shapes = [hd.augment_plan(480, 640, d)[:2] for _, _, d in jobs]
    outs = [torch.empty((r, c, 3), dtype=torch.uint8, device="cuda") for r, c in shapes]
    odesc = [(o.data_ptr(), o.shape[0], o.shape[1], o.shape[1] * 3) for o in outs]
    torch.cuda.synchronize()

    def call():
        hd.augment_frames_device(descs, 3, 0, jobs, odesc)
        hd.check(hd.lib.pbd_synchronize(hd.h))

    wall = median_wall(call)
    ms = []
    stream = torch.cuda.ExternalStream(hd.stream_ptr())
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        hd.augment_frames_device(descs, 3, 0, jobs, odesc)
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    kernel_ms = float(np.median(ms))
    moved = sum(r * c * 3 for r, c in shapes) + len(jobs) * 480 * 640 * 3
    t0 = time.perf_counter()
    ref = A.augment_positives_ref([{"im": f, "points": np.zeros((1, 2))} for f in frames[:REF_FRAMES]], DEGREES, [0],
                                  coef_of=lambda d: A.plan_c(480, 640, d)[2])
    yard = (time.perf_counter() - t0) * 1e3
    equal = all(outs[i].cpu().numpy().tobytes() == ref[i]["im"].tobytes() for i in range(len(ref)))
    hd.close()
    return {"case": f"{NFRAMES} x 640x480x3 uint8, {len(cps)} copies each, one call of {len(jobs)} jobs", "equal_to_yardstick": equal,
            "device_ms": round(kernel_ms, 4), "bytes_moved": moved, "tb_per_s": round(moved / kernel_ms / 1e9, 3),
            "fraction_of_hbm_nominal": round(moved / (kernel_ms * 1e-3) / HBM_NOMINAL, 3),
            "fraction_of_hbm_measured": round(moved / (kernel_ms * 1e-3) / HBM_MEASURED, 3), "device_form_wall_ms": wall,
            "yardstick_host_ms_for_%d_frames" % REF_FRAMES: round(yard, 1), "yardstick_host_ms_scaled": round(yard * NFRAMES / REF_FRAMES, 1),
            "yardstick_over_device_form": round(yard * NFRAMES / REF_FRAMES / wall, 1)}


def latent_line():
    """the latent pass of a train() iteration: the crops of every positive through one latent call per batch of 8"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train_cases
    from partsbaseddetector_amd import train as T
    model, pos, _, kw = train_cases.latent_case()
    pos = list(pos) * LATENT_COPIES
    hd = detector.Handle(model, device=0, max_batch=8)
    hd.set_walk(_lib.WALK_ARGMAX)
    dpos = [dict(p, im=torch.from_numpy(np.array(p["im"])).cuda()) for p in pos]
    torch.cuda.synchronize()

    def run(on_device):
        src = dpos if on_device else pos
        found = 0
        for b in range(0, len(src), 8):
            cb = [T.croppos(p["im"], T.part_boxes(p)) for p in src[b:b + 8]]
            fn = T._detect_latent_device if on_device else T._detect_latent
            found += int(fn(hd, [c for c, _ in cb], [x for _, x in cb], kw["overlap"], None)[1].sum())
        return found

    assert run(True) == run(False)
    t = {True: [], False: []}
    for _ in range(REPS):
        for on_device in (False, True):
            t0 = time.perf_counter()
            run(on_device)
            t[on_device].append((time.perf_counter() - t0) * 1e3)
    hd.close()
    host, dev = float(np.median(t[False])), float(np.median(t[True]))
    return {"case": f"latent pass, {len(pos)} positives of 72x96 in batches of 8, T=float", "host_frames_ms": round(host, 3),
            "device_frames_ms": round(dev, 3), "host_over_device": round(host / dev, 3),
            "host_runs_ms": [round(v, 3) for v in t[False]], "device_runs_ms": [round(v, 3) for v in t[True]]}


def main():
    import torch
    torch.cuda.init()
    args = [a for a in sys.argv[1:] if a != "--latent"]
    out = [augment_line()]
    print(json.dumps(out[0]), flush=True)
    if "--latent" in sys.argv[1:]:
        out.append(latent_line())
        print(json.dumps(out[1]), flush=True)
    if args:
        with open(args[0], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
