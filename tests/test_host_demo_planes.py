"""host/pbd_demo --depth ... --camera ... --remove-planes: the C++ host's organizedMultiplaneSegmentation (pbd_remove_planes)
before clusterObjects, against the numpy yardsticks of partsbaseddetector_amd/pointcloud.py on the demo's own candidates."""
import subprocess

import numpy as np
import pytest

import planes_scenes as S
from partsbaseddetector_amd import model as M, synth
from partsbaseddetector_amd.detector import Candidate
from partsbaseddetector_amd.pointcloud import PointCloudClusterer as PCC, cloud_from_depth
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)
from test_host_demo_pointcloud import same32, write_pfm


@pytest.mark.gpu
def test_demo_remove_planes_lines_match_the_yardsticks(demo, tmp_path):  # noqa: F811
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 240, 320, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    room, cam = S.room(240, 320)
    depth = np.ascontiguousarray(room[:, :, 2])
    dpath = tmp_path / "depth.pfm"
    write_pfm(dpath, np.nan_to_num(depth, nan=0.0))
    depth = np.where(np.isnan(depth), 0.0, depth).astype(np.float32)
    camarg = f"{cam.fx!r},{cam.fy!r},{cam.cx!r},{cam.cy!r}"
    base = [demo, mpath, ipath, "--device-nms", "0.1", "--depth", str(dpath), "--camera", camarg]
    plain = subprocess.run(base, capture_output=True, text=True)
    r = subprocess.run(base + ["--remove-planes"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [ln for ln in lines if not ln.startswith(("plane ", "kept ", "object "))] == \
        [ln for ln in plain.stdout.splitlines() if not ln.startswith("object ")]
    cloud = cloud_from_depth(depth, cam)
    reduced, kept, labels, planes = PCC.organizedMultiplaneSegmentation(cloud)
    pl = [ln.split()[1:] for ln in lines if ln.startswith("plane ")]
    assert len(pl) == len(planes) >= 1
    inl = np.bincount(labels[labels >= 0], minlength=len(planes))
    for k, t in enumerate(pl):
        assert int(t[0]) == k and same32([float(v) for v in t[1:5]], planes[k]) and int(t[5]) == inl[k]
    assert [int(ln.split()[1]) for ln in lines if ln.startswith("kept ")] == [len(kept)]
    _, cands = _parse(r.stdout)
    bl = [[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("box3d_cam ")]
    ol = [ln.split()[1:] for ln in lines if ln.startswith("object ")]
    assert 0 < len(cands) == len(bl) == len(ol)
    wc, wi = PCC.clusterObjects([reduced], np.array(bl), np.zeros(len(bl), np.int32))
    for i, t in enumerate(ol):
        assert int(t[0]) == len(wi[i])
        assert same32([float(v) for v in t[1:]], wc[i])


def test_demo_refuses_remove_planes_without_camera(demo, tmp_path):  # noqa: F811
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    r = subprocess.run([demo, mpath, ipath, "--remove-planes"], capture_output=True, text=True)
    assert r.returncode != 0 and "--remove-planes needs" in r.stderr
