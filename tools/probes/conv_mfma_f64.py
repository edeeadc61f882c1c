"""T = double person model (156 filters of 5x5x32), PBD_CONV_EXACT against PBD_CONV_MFMA_F64, the two modes alternating in one
process: one 640x480 frame per detect() call, and batches of 16 640x480 frames.  Prints milliseconds per frame end to end and
the PBD_K_CONV time of pbd_profile_read (profiling scope on the convolution only), plus the convolution's fp64 FLOP/s
(2 * 800 * filters * cells per frame; the 160-filter padding of the matrix path not counted).
Environment: ROUNDS (default 3); MODES, comma-separated (default "exact,mfma_f64"; one mode for a kernel trace of that mode)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from partsbaseddetector_amd import _lib, synth
from partsbaseddetector_amd.detector import PartsBasedDetector
from partsbaseddetector_amd.model import synthetic_person_model

ROUNDS = int(os.environ.get("ROUNDS", "3"))
MODES = os.environ.get("MODES", "exact,mfma_f64").split(",")
model = synthetic_person_model()
frames = [synth.synthetic_frame(1 + i, 480, 640, 3) for i in range(16)]
dets = {}
for name in MODES:
    mode = {"exact": _lib.CONV_EXACT, "mfma_f64": _lib.CONV_MFMA_F64}[name]
    det = PartsBasedDetector(device=0, dtype=np.float64, conv_mode=mode, max_batch=16)
    det.distributeModel(model)
    dets[name] = det
plan = dets[MODES[0]].hd.plan(480, 640)
cells = int((plan["feat_rows"].astype(np.int64) * plan["feat_cols"]).sum())
flop = 2.0 * 800 * model.flatten().nfilters * cells
print(f"cells per 640x480 frame {cells}, conv {flop / 1e9:.2f} GFLOP per frame", flush=True)


def run(det, batch, reps):
    det.detect_batch(frames[:batch]) if batch > 1 else det.detect(frames[0])        # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        c = det.detect_batch(frames[:batch]) if batch > 1 else det.detect(frames[0])
    ms = (time.perf_counter() - t0) / (reps * batch) * 1e3
    det.hd.profile(2)
    det.detect_batch(frames[:batch]) if batch > 1 else det.detect(frames[0])
    conv_ms = det.hd.profile_read()["k_conv"][0] / batch
    det.hd.profile(0)
    return ms, conv_ms, len(c)


for r in range(ROUNDS):
    for batch, reps in ((1, 20), (16, 3)):
        for name, det in dets.items():
            ms, conv_ms, n = run(det, batch, reps)
            print(f"round {r} batch {batch:2d} {name:9s}: {ms:7.3f} ms/frame end to end, PBD_K_CONV {conv_ms:6.3f} ms/frame "
                  f"({flop / (conv_ms * 1e-3) / 1e12:5.2f} TFLOP/s fp64), {n} candidates", flush=True)
for det in dets.values():
    det.hd.close()
