"""The cases the augmentation tests share (tests/test_augment_cpu.py, tests/test_gpu_augment.py, tests/test_gpu_train_augment.py),
built once per process and never modified.

Frames: the shapes of DESIGN.md section 6r's prototype -- 1 x 1, 2 x 3, 5 x 4, 17 x 9, 48 x 64 -- and 70 x 130, whose rotated
destination rows span more than two waves of 64 lanes.  Every pixel is non-zero
(1..255 before scaling), so the zero fill outside the source can be told from a copied pixel.

The training case: the first 4 positives of tests/trainmodel_cases.py with their points only (a copy carries no boxes:
point_to_box makes them), one angle (15 degrees) and a mirror with the identity permutation (the chain 0 - 1 - 2 has no other
involution that keeps the tree), so 4 copies per positive and 16 positives.  Chosen on the yardstick (trainmodel_ref), first try:
point_to_box's boxes of positive 1 are below minsize, so its four copies are skipped in both latent passes; the other 12 copies,
rotated and mirrored ones included, are found (notfound = []); every (part, type) has a kept positive.  One trainmodel_ref run
takes 3.8 s on the development machine's CPU.
"""
import functools

import numpy as np

import trainmodel_cases as TC

SHAPES = ((1, 1), (2, 3), (5, 4), (17, 9), (48, 64), (70, 130))
DEGREES = (0.0, 90.0, 180.0, 270.0, 7.5, -7.5, 15.0, -15.0, 45.0, 33.3)
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)

NPOS = 4
AUGMENT = {"degrees": (15.0,), "mirror": [0, 1, 2]}
COPIES = 4          # (no mirror, mirror) x (0, 15)


@functools.lru_cache(maxsize=None)
def frames(dtype, cn):
    """one frame per shape of SHAPES, rows x cols x cn, no zero pixel"""
    rng = np.random.default_rng(17 + cn)
    out = []
    for r, c in SHAPES:
        base = rng.integers(1, 256, (r, c, cn)).astype(np.int64)
        if np.dtype(dtype) == np.uint8:
            f = base.astype(np.uint8)
        elif np.dtype(dtype) == np.uint16:
            f = (base * 257 - 1).astype(np.uint16)                     # up to 65534, never 0
        else:
            f = (base.astype(dtype) - dtype(100.5)) / dtype(7)         # both signs, never 0
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


def all_jobs(nframes=len(SHAPES), skip=()):
    """(frame, mirror, degrees) for every frame not in `skip`, every angle of DEGREES, mirror off and on"""
    return [(f, m, d) for f in range(nframes) if f not in skip for d in DEGREES for m in (False, True)]


@functools.lru_cache(maxsize=None)
def train_case():
    """(pos, neg, keywords of trainmodel, the augment argument)"""
    pos, neg, kw = TC.case()
    pos = [dict(im=p["im"], points=p["points"]) for p in pos[:NPOS]]
    return pos, neg, kw, AUGMENT


@functools.lru_cache(maxsize=None)
def ref_run():
    """trainmodel_ref on the training case: (model, info)"""
    from partsbaseddetector_amd import trainmodel as TM
    pos, neg, kw, aug = train_case()
    return TM.trainmodel_ref(pos, neg, dtype=np.float32, augment=aug, **kw)
