"""host/pbd_demo --marginal-pose PART (PartsBasedDetector<T>::maxMarginals / marginalPoses, include/pbd_host.hpp): the usage text
names the flag and the runs it cannot serve are refused (no GPU needed), and on the GPU the demo prints the level, cell and score
bits of the part's best max-marginal by the numpy rule (partsbaseddetector_amd/marginals.py) on the oracle's responses, and the
decoded pose's root."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import examples as E
from partsbaseddetector_amd import filestorage as FS
from partsbaseddetector_amd import marginals as MG
from partsbaseddetector_amd import model as M, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "host", "pbd_demo")


@pytest.fixture(scope="module")
def demo():
    from partsbaseddetector_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])
    return DEMO


def test_usage_names_the_flag(demo):
    r = subprocess.run([demo], capture_output=True, text=True)
    assert r.returncode != 0 and "--marginal-pose" in r.stderr


@pytest.mark.parametrize("args", [["--staged"], ["--stream", "2", "3"], ["--also", "other.ppm"]], ids=["staged", "stream", "also"])
def test_runs_without_one_resident_result_are_refused_before_anything_is_read(demo, args):
    r = subprocess.run([demo, "no_model.yml", "no_image.ppm", "--marginal-pose", "1"] + args, capture_output=True, text=True)
    assert r.returncode != 0 and "--marginal-pose" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--double"]], ids=["float", "double"])
def test_demo_prints_the_best_cell_of_the_part_and_its_pose(demo, tmp_path, flags):
    dtype = np.float64 if "--double" in flags else np.float32
    mpath, ipath = str(tmp_path / "model.yml"), str(tmp_path / "frame.ppm")
    FS.serialize(M.synthetic_tiny_model(thresh=0.6), mpath)
    flat = FS.deserialize(mpath).flatten()
    im = synth.synthetic_frame(31, 72, 96, 3)
    with open(ipath, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]))
        fh.write(np.ascontiguousarray(im[:, :, ::-1]).tobytes())          # PPM stores RGB; the demo hands BGR to detect()
    part = 2
    r = subprocess.run([demo, mpath, ipath, "--marginal-pose", str(part), "--top", "2"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("marginal_pose ")]
    assert len(at) == 1
    t = lines[at[0]].split()
    pose = [ln.split() for ln in lines[at[0] + 1:] if ln.startswith("cand ")]
    assert len(pose) == 1
    # the rule: the first largest value over (level, type, cell) of the part's planes
    fm = E.FrameMaps(flat, im, dtype)
    g0, g1 = int(flat.mix_offset[part]), int(flat.mix_offset[part + 1])
    best = None
    for lvl in range(len(fm.feats)):
        mm, _, Jx, Jy, Jk = MG.max_marginals(flat, 0, fm.resp(lvl))
        blk = mm[g0:g1]
        if blk.size and (best is None or blk.max() > best[0]):
            m, y, x = np.unravel_index(int(np.argmax(blk)), blk.shape)
            best = (blk.max(), lvl, int(m), int(x), int(y), (mm, Jx, Jy, Jk))
    assert [int(v) for v in t[1:5]] == [part, best[1], best[3], best[4]]
    assert np.float32(float.fromhex(t[5])).tobytes() == np.float32(best[0]).tobytes()
    mm, Jx, Jy, Jk = best[5]
    IxRaw, IyRaw, Ik, _, _ = E.raw_maps(flat, 0, fm.resp(best[1]))
    place, rec = MG.decode(flat, 0, best[1], part, best[2], best[3], best[4], mm, Jx, Jy, Jk, IxRaw, IyRaw, Ik, 1.0, dtype=dtype)
    assert [int(v) for v in pose[0][1:5]] == [best[1], 0, place[0][1], place[0][0]]
