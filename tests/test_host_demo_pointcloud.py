"""host/pbd_demo --depth ... --camera fx,fy,cx,cy: the C++ host's PartsBasedDetector<T>::computeBoundingBoxes /
clusterObjects (pbd_boxes3d_camera, pbd_cluster_objects) against the numpy yardsticks of partsbaseddetector_amd/pointcloud.py
on the demo's own reported candidates; without --camera the output is unchanged."""
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, synth
from partsbaseddetector_amd.detector import Candidate
from partsbaseddetector_amd.pointcloud import PinholeCamera, PointCloudClusterer as PCC, cloud_from_depth
from test_host_demo import _parse, _write_inputs, demo  # noqa: F401  (fixture)


def same32(a, b):
    """float32 bit patterns equal; NaN equals NaN (the text "nan" does not keep a NaN's sign or payload)"""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def write_pfm(path, depth):
    """grey PFM: little-endian (negative scale), rows bottom to top"""
    h, w = depth.shape
    path.write_bytes(b"Pf\n%d %d\n-1.0\n" % (w, h) + np.ascontiguousarray(depth[::-1]).astype("<f4").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,flags", [("pfm", ["--device-nms", "0.1"]), ("pfm", ["--double", "--nms", "0.1", "--top", "3"]),
                                        ("pgm", ["--device-nms", "0.1"])])
def test_demo_camera_lines_match_the_yardsticks(demo, tmp_path, kind, flags):  # noqa: F811
    """pfm: float metres, where the clustering forms clusters; pgm: 16-bit millimetres converted unscaled, as cv_bridge does
    (integer steps make boundingBox3D's walk stop on a plateau, so its boxes mostly have zero depth and no points)"""
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    if kind == "pfm":
        depth = synth.synthetic_depth(21, 160, 120, np.float32)
        dpath = tmp_path / "depth.pfm"
        write_pfm(dpath, depth)
    else:
        depth16 = synth.synthetic_depth(21, 160, 120, np.uint16)
        dpath = tmp_path / "depth.pgm"
        dpath.write_bytes(b"P5\n120 160\n65535\n" + depth16.astype(">u2").tobytes())
        depth = depth16.astype(np.float32)
    cam = PinholeCamera(600.0, 590.5, 59.5, 80.25)
    base = [demo, mpath, ipath] + flags + ["--depth", str(dpath)]
    plain = subprocess.run(base, capture_output=True, text=True)
    r = subprocess.run(base + ["--camera", "600,590.5,59.5,80.25"], capture_output=True, text=True)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    new = ("box3d_cam ", "centres ", "object ")
    assert [ln for ln in lines if not ln.startswith(new)] == plain.stdout.splitlines()
    _, cands = _parse(r.stdout)
    bl = [[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("box3d_cam ")]
    cl = [ln.split()[1:] for ln in lines if ln.startswith("centres ")]
    ol = [ln.split()[1:] for ln in lines if ln.startswith("object ")]
    assert 0 < len(cands) == len(bl) == len(cl) == len(ol)
    cs = [Candidate(parts=parts, confidence=np.zeros(len(parts), np.float32), component=0) for _, _, parts in cands]
    for c in cs:
        c.frame = 0
    boxes, centres, ncent, _ = PCC.computeBoundingBoxes(cs, [im.shape[:2]], [depth], [cam])
    np.testing.assert_array_equal(np.array(bl), boxes)                          # %.17g round-trips a double
    for i, t in enumerate(cl):
        assert int(t[0]) == ncent[i]
        got = np.array([float(v) for v in t[1:]], np.float32).reshape(-1, 3)     # %.9g round-trips a float
        assert same32(got, centres[i, :ncent[i]])
    wc, wi = PCC.clusterObjects([cloud_from_depth(depth, cam)], boxes, np.zeros(len(boxes), np.int32))
    if kind == "pfm":
        assert any(len(v) > 1 for v in wi)
    for i, t in enumerate(ol):
        assert int(t[0]) == len(wi[i])
        assert same32([float(v) for v in t[1:]], wc[i])
