"""Time of pbd_part_scores_device on the records of the 64 x 640x480 bench workload (synthetic person model, frames of seeds
1..64): the 6303 unsuppressed records and the 218 pbd_set_nms(0.1) keeps.  The yardstick is pbd_examples_device on the same
records in the same process, the only way to a part's score before (it walks the same maps and moves the 800 values of every
part's feature window where this moves one response).  Both are timed between two events on the handle's stream, the two calls
alternating, after a warm-up of each; median / min / max of --reps.  Also counted, in arg-max walk mode: the records whose root
message has the bits of the record's score (guarantee 1 of include/pbd.h: all of them).  One JSON line per case; with an
argument, also written to that file.

    python tools/probes/part_scores_cost.py [out.jsonl] [--reps N]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

B, ROWS, COLS = 64, 480, 640


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    import torch
    torch.cuda.init()
    args = [a for a in sys.argv[1:]]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
    path = args[0] if args and not args[0].startswith("--") else None
    out = []
    frames = np.stack([synth.synthetic_frame(i + 1, ROWS, COLS) for i in range(B)])
    d_frames = torch.from_numpy(frames).cuda()
    for dtype in (np.float32, np.float64):
        real = _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64
        tdt = torch.float32 if dtype == np.float32 else torch.float64
        cap = 1 << 16
        hd = detector.Handle(M.synthetic_person_model(), device=0, max_batch=B, max_candidates=cap, real_type=real)
        stream = torch.cuda.ExternalStream(hd.stream_ptr())
        mp = (hd.stride - 8) // 4
        hw, vw = hd.example_stride()
        pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def detect():
            hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, B, d_frames.data_ptr(), ROWS, COLS, 3, 0, pay.data_ptr(), cap))
            hd.check(hd.lib.pbd_synchronize(hd.h))
            return int(pay[0].item())

        for nms in (None, 0.1):
            hd.set_walk(_lib.WALK_REFERENCE)
            hd.set_nms(nms)
            n = detect()
            assert 0 < n <= cap
            d_st = torch.empty(n, dtype=torch.int32, device="cuda")
            d_pl = torch.empty((n, mp, 3), dtype=torch.int32, device="cuda")
            d_sc = torch.empty((n, mp, 4), dtype=tdt, device="cuda")
            d_hdr = torch.empty((n, hw), dtype=torch.int32, device="cuda")
            d_val = torch.empty((n, vw), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            calls = {"part_scores": lambda: hd.part_scores_device(pay.data_ptr(), n, 0, d_st.data_ptr(), d_pl.data_ptr(), d_sc.data_ptr()),
                     "examples": lambda: hd.examples_device(pay.data_ptr(), n, 0, d_hdr.data_ptr(), d_val.data_ptr())}
            ms = {k: [] for k in calls}
            for rep in range(-3, reps):                    # three warm-up rounds
                for k, call in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    call()
                    b.record(stream)
                    b.synchronize()
                    if rep >= 0:
                        ms[k].append(a.elapsed_time(b))
            assert int((d_st != mp).sum().item()) == 0
            # arg-max walk: the root's message is the record's score, bit for bit
            hd.set_walk(_lib.WALK_ARGMAX)
            k = min(detect(), n)                           # the suppression sees other boxes: the count may differ
            hd.part_scores_device(pay.data_ptr(), k, 0, d_st.data_ptr(), d_pl.data_ptr(), d_sc.data_ptr())
            hd.check(hd.lib.pbd_synchronize(hd.h))
            rec = pay[1:1 + k * hd.stride].view(k, hd.stride)
            same = int((d_sc[:k, 0, 1].to(torch.float32).contiguous().view(torch.int32) == rec[:, 5]).sum().item())
            line = {"case": f"{B} x {COLS}x{ROWS}, person model, T={np.dtype(dtype).name}, "
                            + ("NMS off" if nms is None else f"pbd_set_nms({nms})"),
                    "records": n, "reps": reps, "part_scores_device_ms": stats(ms["part_scores"]),
                    "examples_device_ms": stats(ms["examples"]),
                    "examples_over_part_scores": round(float(np.median(ms["examples"]) / np.median(ms["part_scores"])), 1),
                    "bytes_written_part_scores": n * mp * (3 * 4 + 4 * np.dtype(dtype).itemsize) + 4 * n,
                    "bytes_written_examples": n * (hw * 4 + vw * np.dtype(dtype).itemsize),
                    "argmax_root_message_equals_score": f"{same} of {k}"}
            print(json.dumps(line), flush=True)
            out.append(line)
        hd.close()
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
