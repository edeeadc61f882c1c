"""PBD_CONV_FMA against PBD_CONV_MFMA_ANY (5) and PBD_CONV_MFMA_F16_ANY (6) on banks the 5 x 5 matrix modes refuse, the three
handles alternating in one process over a warmed window.  Per case: 640 x 480 frames, one per detect() call and batches of 16;
the convolution's time is PBD_K_CONV of pbd_profile_read with the profiling scope on the convolution only (the median of
REPS profiled calls per handle, the handles taking turns inside every repetition), next to the end-to-end time per frame
(host clock around calls that end in a synchronise, profiling off).

Cases: 156-filter person-layout banks of side 1, 2, 3, 7, 9, 12; the [3, 4, 7] mixed bank; a 5-filter 31 x 31 bank; and the all-5 x 5
person model in modes 2 and 5, which run the same kernel and must agree.

Printed per line: useful TFLOP/s (2 k k 32 products per filter and cell), executed matrix TFLOP/s (what the MFMAs issue: three
per product tile in bf16, M-tiles of 32 filters, whole 32 x 8 pixel tiles, pad taps), LDS per workgroup, resident workgroups
per CU.  Environment: REPS (default 7), CASES (comma-separated names, default all)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from partsbaseddetector_amd import _lib, synth  # noqa: E402
from partsbaseddetector_amd import model as MD  # noqa: E402
from partsbaseddetector_amd.detector import PartsBasedDetector  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
HIGH = 1e9           # no root passes: the step is the pyramid, the convolution and the dynamic program, no walks
CASES = {
    "k1": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=1, thresh=HIGH, name="p1"),
    "k2": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=2, thresh=HIGH, name="p2"),
    "k3": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=3, thresh=HIGH, name="p3"),
    "k7": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=7, thresh=HIGH, name="p7"),
    "k9": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=9, thresh=HIGH, name="p9"),
    "k12": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=12, thresh=HIGH, name="p12"),
    "mixed_3_4_7": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=[3, 4, 7], thresh=HIGH, name="pm"),
    "k31x5": lambda: MD.synthetic_model(seed=26, pa=[0, 1, 1, 2, 2], nmix=1, ksize=31, thresh=HIGH, name="p31"),
    "k5_person": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=5, thresh=HIGH, name="p5"),
    "k5_person_rev": lambda: MD.synthetic_model(seed=26, pa=synth.PERSON_PA, nmix=6, ksize=5, thresh=HIGH, name="p5"),
}
MODES = {"fma": _lib.CONV_FMA, "any": _lib.CONV_MFMA_ANY, "any16": _lib.CONV_MFMA_F16_ANY, "mfma": _lib.CONV_MFMA}
frames = [synth.synthetic_frame(1 + i, 480, 640, 3) for i in range(16)]
lib = _lib.load()
lib.pbd_debug_conv_any.argtypes = [C.c_int, C.c_int, C.c_int]


def work(det, flat, f16):
    """(useful, executed) FLOP of one frame's convolution.  `executed` follows k_conv_mfma_any's rule (steps per channel block,
    M-tiles of 32 filters, 32 x 8 pixel tiles).  The 5 x 5 person cases run k_conv_mfma<5> instead (passes of 160 filters, 256-
    pixel tiles of three shapes): for 156 filters and 32 channels in 2 KK steps both rules give the same count up to the
    tiles' edge pixels, so their lines are comparable but are that kernel's only approximately."""
    plan = det.hd.plan(480, 640)
    rows, cols = plan["feat_rows"].astype(np.int64), plan["feat_cols"].astype(np.int64)
    cells = int((rows * cols).sum())
    tiles = int((((rows + 7) // 8) * ((cols + 31) // 32))[(rows * cols) > 0].sum())
    useful = executed = 0.0
    ks = np.asarray(flat.filter_ksize)
    for k in sorted(set(int(v) for v in ks)):
        nf = int((ks == k).sum())
        cb = lib.pbd_debug_conv_any(k, int(f16), 2)
        steps = {32: 2 * k * k, 16: k * k, 8: (k * k + 1) // 2}[cb] * (32 // cb)
        useful += 2.0 * k * k * 32 * nf * cells
        executed += 2.0 * (1 if f16 else 3) * ((nf + 31) // 32 * 32) * (steps * 16) * (tiles * 256)
    return useful, executed


def call(det, batch):
    return det.detect_batch(frames[:batch]) if batch > 1 else det.detect(frames[0])


def main():
    names = os.environ.get("CASES", ",".join(CASES)).split(",")
    for cname in names:
        model = CASES[cname]()
        flat = model.flatten()
        # (the 5 x 5 model twice, the two handles created and run in either order: they run the same kernel)
        modes = {"k5_person": ["mfma", "any"], "k5_person_rev": ["any", "mfma"]}.get(cname, ["fma", "any", "any16"])
        dets = {}
        for m in modes:
            dets[m] = PartsBasedDetector(device=0, conv_mode=MODES[m], max_batch=16)
            dets[m].distributeModel(model)
        sides = sorted(set(int(v) for v in flat.filter_ksize))
        for m in modes:
            if m in ("any", "any16"):
                info = ", ".join(f"k={k}: {lib.pbd_debug_conv_any(k, int(m == 'any16'), 2)} channels, "
                                 f"{lib.pbd_debug_conv_any(k, int(m == 'any16'), 1)} B LDS, "
                                 f"{lib.pbd_debug_conv_any(k, int(m == 'any16'), 0)} workgroups/CU" for k in sides)
                print(f"{cname} {m}: {flat.nfilters} filters; {info}", flush=True)
        for batch in (1, 16):
            for det in dets.values():                     # warm every shape of the window
                call(det, batch); call(det, batch)
            conv = {m: [] for m in modes}
            e2e = {m: [] for m in modes}
            for _ in range(REPS):
                for m, det in dets.items():               # the handles take turns
                    t0 = time.perf_counter()
                    for _ in range(3):
                        call(det, batch)
                    e2e[m].append((time.perf_counter() - t0) / (3 * batch) * 1e3)
                    det.hd.profile(2)
                    call(det, batch)
                    conv[m].append(det.hd.profile_read()["k_conv"][0] / batch)
                    det.hd.profile(0)
            base = float(np.median(conv[modes[0]]))
            for m, det in dets.items():
                c, lo, hi = float(np.median(conv[m])), min(conv[m]), max(conv[m])
                useful, executed = work(det, flat, m == "any16")
                line = (f"{cname:12s} batch {batch:2d} {m:6s}: conv {c:8.3f} ms/frame (min {lo:.3f}, max {hi:.3f}), "
                        f"{base / c:5.2f} x {modes[0]}, useful {useful / (c * 1e-3) / 1e12:6.2f} TFLOP/s")
                if m != "fma":
                    line += f", executed {executed / (c * 1e-3) / 1e12:6.2f} TFLOP/s on the matrix cores"
                line += f"; end to end {float(np.median(e2e[m])):8.3f} ms/frame"
                print(line, flush=True)
        for det in dets.values():
            det.hd.close()


if __name__ == "__main__":
    main()
