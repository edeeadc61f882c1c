"""Shared inputs of the pipelined / pooled detection tests (test_gpu_pipeline.py, test_host_stream.py, test_pipeline_cases_cpu.py),
built once per process.

Every expected list is the CPU oracle's (`oracle.detect`, float, per frame), laid out as the int32 records of include/pbd.h in
the order of pbd_detect_batch: (frame, level, component, root_y, root_x), `frame` = index in the batch.  With the
post-processing stage on, the Python mirror of the callers' post-step (Candidate.sort + Candidate.nonMaximaSuppression) is applied
to those records.  Nothing here comes from the code under test.

The frames differ in size and in how many candidates they hold, on purpose:
  A     96 x 128   hundreds of candidates (more than 64)
  B     64 x  80   fewer than 1024
  C*   120 x 160   three frames that together exceed 1024: the speculative read-back's first guess is too short
  Z     96 x 128   constant 128: a handful (0 < n <= 8)
  Z64   64 x  80   constant 128: a handful (n <= 8)
A batch holds frames of one size (`pair`: A and a second frame of A's size from another seed).
"""
import functools

import numpy as np

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import synth
from partsbaseddetector_amd.detector import Candidate

THRESH = 0.6
MAX_BATCH = 3
MAX_CANDIDATES = 1 << 16
GUESS = 1024            # records the first speculative read-back of a handle covers


@functools.lru_cache(maxsize=None)
def model():
    return M.synthetic_tiny_model(thresh=THRESH)


@functools.lru_cache(maxsize=None)
def frames():
    """name -> uint8 frame (rows, cols, 3); never modified by a test (tests copy what they overwrite)"""
    f = {
        "A": synth.synthetic_frame(5, 96, 128, 3),
        "A2": synth.synthetic_frame(15, 96, 128, 3),
        "B": synth.synthetic_frame(6, 64, 80, 3),
        "C": synth.synthetic_frame(7, 120, 160, 3),
        "C1": synth.synthetic_frame(17, 120, 160, 3),
        "C2": synth.synthetic_frame(27, 120, 160, 3),
        "Z": np.full((96, 128, 3), 128, np.uint8),
        "Z64": np.full((64, 80, 3), 128, np.uint8),
    }
    for a in f.values():
        a.setflags(write=False)
    return f


BATCHES = {
    "small": ("B",),
    "large": ("C", "C1", "C2"),
    "blank": ("Z",),
    "pair": ("A", "A2"),
}


def batch_frames(name):
    return [frames()[k] for k in BATCHES[name]]


@functools.lru_cache(maxsize=None)
def stride():
    return 8 + 4 * model().flatten().max_parts


@functools.lru_cache(maxsize=None)
def frame_records(name):
    """the oracle's records of one frame, `frame` = 0, in (level, component, root_y, root_x) order"""
    from oracle import oracle
    oracle.build()
    want = oracle.detect(model().flatten(), frames()[name])
    rec = np.zeros((len(want), stride()), np.int32)
    for i, w in enumerate(want):
        parts = np.asarray(w["parts"], np.int32).reshape(-1, 4)
        rec[i, :8] = (0, w["component"], w["level"], w["root_x"], w["root_y"], 0, len(parts), 0)
        rec[i, 5] = np.float32(w["score"]).view(np.int32)
        rec[i, 8:8 + parts.size] = parts.ravel()
    keys = [tuple(r[[2, 1, 4, 3]]) for r in rec]
    assert keys == sorted(keys)
    rec.setflags(write=False)
    return rec


def records_of(names):
    """the oracle's records of a batch of named frames, `frame` = index in the batch"""
    out = []
    for i, k in enumerate(names):
        r = frame_records(k).copy()
        r[:, 0] = i
        out.append(r)
    return np.concatenate(out, axis=0) if out else np.zeros((0, stride()), np.int32)


@functools.lru_cache(maxsize=None)
def batch_records(name):
    rec = records_of(BATCHES[name])
    rec.setflags(write=False)
    return rec


def mirror(rec, rows, cols, overlap):
    """the callers' post-step on (n, stride) records, frame by frame: Candidate.sort, then Candidate.nonMaximaSuppression
    (as tests/test_gpu_nms.py::mirror); returns the kept records in the kept order"""
    keep = []
    for f in np.unique(rec[:, 0]):
        cands = []
        for i in np.nonzero(rec[:, 0] == f)[0]:
            r = rec[i]
            npart = int(r[6])
            conf = np.zeros(npart, np.float32)
            conf[0] = r[5:6].view(np.float32)[0]
            c = Candidate(parts=r[8:8 + 4 * npart].reshape(npart, 4), confidence=conf, component=int(r[1]), frame=int(f))
            c.row = int(i)
            cands.append(c)
        Candidate.sort(cands)
        Candidate.nonMaximaSuppression((rows, cols), cands, float(np.float32(overlap)))
        keep.extend(c.row for c in cands)
    return rec[np.array(keep, np.int64)] if keep else np.zeros((0, rec.shape[1]), np.int32)
