"""Kernel time of testing a model on the device -- pbd_part_nms_device, pbd_best_overlap_device, pbd_eval_pck_device,
pbd_eval_apk_device, each through pbd_profile_read -- on the unsuppressed list of a 64 x 640x480 step of the synthetic person
model, next to the numpy yardstick (partsbaseddetector_amd/evaluation.py) timed on the host on the same list.  Prints one JSON line
per threshold; with an argument, also writes them to that file.

    python tools/probes/eval_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, detector, synth  # noqa: E402
from partsbaseddetector_amd import evaluation as ev  # noqa: E402
from partsbaseddetector_amd import model as M  # noqa: E402

NMS = ["k_ev_nms_select", "k_ev_nms_pairs", "k_ev_nms_greedy", "k_ev_nms_emit"]
APK = ["k_ev_apk_rank", "k_ev_apk_close", "k_ev_apk_ap"]


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


def host_s(fn):
    t = time.perf_counter()
    out = fn()
    return round(time.perf_counter() - t, 3), out


def main():
    import torch
    torch.cuda.init()
    out = []
    nf, cap, npart = 64, 1 << 18, 26
    frames = np.stack([synth.synthetic_frame(s, 480, 640) for s in range(nf)])
    d_frames = torch.from_numpy(frames).cuda()
    for thresh in (M.PERSON_THRESH, M.PERSON_THRESH - 1.0, M.PERSON_THRESH - 2.0):
        hd = detector.Handle(M.synthetic_person_model(thresh=thresh), device=0, max_batch=nf, max_candidates=cap)
        pay = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
        kept = torch.zeros(1 + cap * hd.stride, dtype=torch.int32, device="cuda")
        hd.check(hd.lib.pbd_detect_batch_device_out(hd.h, nf, d_frames.data_ptr(), 480, 640, 3, 0, pay.data_ptr(), cap))
        hd.check(hd.lib.pbd_synchronize(hd.h))
        found = int(pay[0].item())
        n = min(found, cap)
        pay[0] = n                      # a truncated list is refused; the probe times the first `cap` records as a list
        torch.cuda.synchronize()
        raw = pay[1:1 + n * hd.stride].cpu().numpy().reshape(n, hd.stride)
        per_frame = np.bincount(raw[:, 0], minlength=nf)
        # ground truth: per frame the centre hull and the centres of its highest-scoring record, one instance per frame
        gtb = np.full((nf, 4), np.nan)
        gtp = np.zeros((nf, npart, 2))
        for f in range(nf):
            idx = np.flatnonzero(raw[:, 0] == f)
            if len(idx):
                c = ev.centres(raw[idx[np.argmax(ev.scores(raw[idx]))]][None], npart)[0]
                gtb[f] = [c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()]
                gtp[f] = c + 2.0
        scale = np.full(nf, 10.0)
        gt_offset = np.arange(nf + 1, dtype=np.int32)

        nms_ms, nms_per = kernel_ms(hd, NMS, lambda: hd.part_nms_device(nf, 0.3, 1000, pay.data_ptr(), cap, 0, kept.data_ptr(), cap))
        nkept = int(kept[0].item())
        best = torch.zeros(nf * (hd.stride + 1), dtype=torch.int32, device="cuda")
        d_found = best.data_ptr() + 4 * nf * hd.stride
        best_ms, _ = kernel_ms(hd, ["k_ev_best"], lambda: hd.best_overlap_device(gtb, 0.3, pay.data_ptr(), cap, 0, best.data_ptr(), d_found))
        d_pck = torch.zeros(npart * (nf + 1), dtype=torch.float64, device="cuda")
        pck_ms, _ = kernel_ms(hd, ["k_ev_pck"], lambda: hd.eval_pck_device(nf, best.data_ptr(), d_found, gtp, scale, 0.5, d_pck.data_ptr(),
                                                                           d_pck.data_ptr() + 8 * npart))
        d_apk = torch.zeros(npart, dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        apk_ms, apk_per = kernel_ms(hd, APK, lambda: hd.eval_apk_device(gt_offset, gtp, scale, 0.5, kept.data_ptr(), cap, 0, d_apk.data_ptr(),
                                                                        None, None, status.data_ptr()))
        # the yardstick on the host, on the same lists (and the results compared while we are here)
        t_nms, wkept = host_s(lambda: ev.part_nms(raw, nf, npart, 0.3))
        t_best, (wbest, wfound) = host_s(lambda: ev.best_overlap(raw, nf, npart, gtb, 0.3))
        t_pck, (wpck, _) = host_s(lambda: ev.eval_pck(wbest, wfound, npart, gtp, scale, 0.5))
        t_apk, (wapk, _, _) = host_s(lambda: ev.eval_apk(wkept, nf, npart, gt_offset, gtp, scale, 0.5))
        equal = bool(nkept == len(wkept) and kept[1:1 + nkept * hd.stride].cpu().numpy().tobytes() == wkept.tobytes() and
                     best[:nf * hd.stride].cpu().numpy().tobytes() == wbest.tobytes() and
                     d_pck[:npart].cpu().numpy().tobytes() == wpck.tobytes() and d_apk.cpu().numpy().tobytes() == wapk.tobytes())
        rec = {"case": f"64 x 640x480, person model, thresh {thresh:.2f}", "found": found, "records": n,
               "records_per_frame_max": int(per_frame.max()), "frames_above_1000": int((per_frame > 1000).sum()), "kept": nkept,
               "part_nms_ms": nms_ms, "part_nms_per_kernel_ms": nms_per, "best_overlap_ms": best_ms, "pck_ms": pck_ms,
               "apk_ms": apk_ms, "apk_per_kernel_ms": apk_per,
               "numpy_s": {"part_nms": t_nms, "best_overlap": t_best, "pck": t_pck, "apk": t_apk}, "equals_numpy": equal}
        print(json.dumps(rec))
        out.append(rec)
        hd.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
