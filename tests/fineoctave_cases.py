"""Built inputs of the fine-octave tests (tests/test_fineoctave_cpu.py, tests/test_gpu_fineoctave.py): the planted object."""
import numpy as np

from partsbaseddetector_amd import model as M, synth

PLANT_SEED = 3
PLANT_AT = (18, 26)          # (y, x) of the pasted patch's corner in the frame
PLANT_SHAPE = (64, 80)
PLANT_THRESH = 13.0          # between the best score with the octave off (10.63) and on (15.28), float and double alike


def planted(oracle, seed=PLANT_SEED, sbin=4, k=5, interval=5):
    """(model, frame, box): a one-part model whose k x k filter is the HOG of a smooth textured patch of (k + 2) * sbin pixels a
    side, and a flat frame with that patch pasted at HALF size at PLANT_AT.  box = (x, y, side) of the pasted patch's interior,
    the pixels its k x k cells at bin size sbin / 2 cover (HOG drops one block on every side)."""
    side = (k + 2) * sbin
    patch = oracle.resize_linear_u8(synth.synthetic_frame(seed, 7, 7, 3), side, side)
    filt = oracle.hog_features(patch, sbin, dtype=np.float64)
    assert filt.shape == (k, k * 32)
    m = M.Model(name="planted", interval=interval, thresh=PLANT_THRESH, sbin=sbin)
    m.filtersw = [filt]
    m.biasw = [0.0]
    m.filterid, m.biasid, m.defid, m.parentid = [[[0]]], [[[0]]], [[[]]], [[-1]]
    m.validate()
    im = np.full(PLANT_SHAPE + (3,), 128, np.uint8)
    y, x = PLANT_AT
    im[y:y + side // 2, x:x + side // 2] = oracle.resize_linear_u8(patch, side // 2, side // 2)
    return m, im, (x + sbin // 2, y + sbin // 2, k * sbin // 2)
