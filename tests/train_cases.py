"""The two training cases train() and train_ref() are compared on (tests/test_train_cpu.py, tests/test_gpu_train.py), built once
per process.  Seeds, capacity and pass count were chosen on the yardstick (train_ref) so that one run reaches every branch of the
loop the tests assert: every positive found, a batch that optimises and prunes because the cache is full, a batch that makes
one pass, and records the payload had no room for.

latent case: the tiny model (3 parts x 2 mixtures), 4 positives of 72 x 96 whose ground-truth boxes are the part boxes of a
  seeded record of the untrained model on that frame (a placement that passes every overlap mask exists, so each is found),
  3 negatives of 72 x 96, 60 x 80 and 72 x 96, at most 30 passes per optimisation, seed 0.  Capacity 480: at C = 0.002 the
  weights stay small, nearly every root cell of a negative scores above -1 (622 records on 72 x 96, about 400 on 60 x 80), and
  at a capacity near 96 every batch fills the cache and takes the opt + prune branch (tried: 96, 100, 110, 128, five seed sets,
  C up to 20).  At 480 the first frame overflows the room (146 records dropped, n == capacity, opt + prune), the second fits
  and makes one pass, the third finds only the few records the updated model still lets through.
warp case: a one-part 5 x 5 model, 6 boxes of which box 3 (12 x 16 pixels) is below minsize = 400, 2 negatives, capacity 64.
"""
import functools

import numpy as np

from partsbaseddetector_amd import model as M
from partsbaseddetector_amd import synth

LATENT = dict(capacity=480, max_passes=30, seed=0, overlap=0.6, neg_interval=2, neg_batch=1, tol=0.05)
WARP = dict(capacity=64, max_passes=30, seed=0, neg_interval=2, neg_batch=1, tol=0.05)
POS_SEEDS = (31, 32, 33, 34)
NEG_FRAMES = ((41, 72, 96), (42, 60, 80), (43, 72, 96))


def _inclusive(parts):
    return np.array([(x, y, x + w, y + h) for x, y, w, h in parts], np.int32)


@functools.lru_cache(maxsize=None)
def latent_case():
    """(model, pos, neg, keywords)"""
    from oracle import oracle
    oracle.build()
    model = M.synthetic_tiny_model(thresh=-0.5)
    flat = model.flatten()
    pos = []
    for s in POS_SEEDS:
        im = synth.synthetic_frame(s, 72, 96)
        recs = [r for r in oracle.detect(flat, im)
                if all((w + 1) * (h + 1) >= 400 and x >= 0 and y >= 0 and x + w < 96 and y + h < 72 for x, y, w, h in r["parts"])]
        r = recs[int(np.random.default_rng(s).integers(len(recs)))]
        pos.append({"im": im, "boxes": _inclusive(r["parts"])})
    neg = [synth.synthetic_frame(s, r, c) for s, r, c in NEG_FRAMES]
    return model, pos, neg, dict(LATENT)


@functools.lru_cache(maxsize=None)
def warp_case():
    model = M.synthetic_model(seed=4, pa=[0], nmix=1, ksize=5, interval=3, thresh=-1.0, name="synthetic_one_part")
    boxes = [(10, 8, 49, 47), (30, 20, 61, 59), (5, 5, 44, 36), (40, 30, 51, 45), (0, 0, 39, 39), (50, 25, 95, 70)]
    pos = [{"im": synth.synthetic_frame(50 + i, 72, 96), "boxes": np.array([b], np.int32)} for i, b in enumerate(boxes)]
    neg = [synth.synthetic_frame(61, 60, 80), synth.synthetic_frame(62, 72, 96)]
    return model, pos, neg, dict(WARP)
