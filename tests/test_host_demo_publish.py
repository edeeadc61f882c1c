"""host/pbd_demo --mask / --masked / --poses: the C++ host's PartsBasedDetector<T>::mask and partPoses (pbd_candidate_mask,
pbd_part_poses) against the numpy yardsticks of partsbaseddetector_amd/publish.py on the demo's own reported candidates; the new
pbd_bind.hpp / pbd_host.hpp lines and the cv::Mat adapter calls compile without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import model as M, publish, synth
from partsbaseddetector_amd.detector import Candidate
from partsbaseddetector_amd.pointcloud import PinholeCamera, PointCloudClusterer as PCC
from test_host_demo import ROOT, _parse, _write_inputs, demo  # noqa: F401  (fixture)

DOUBLES = os.path.join(ROOT, "tests", "adapter_doubles")
DOUBLES_DEPTH = os.path.join(ROOT, "tests", "adapter_doubles_depth")


def read_pnm(path):
    data = open(path, "rb").read()
    magic, w, h, mx, rest = data.split(maxsplit=4)
    cn = 3 if magic == b"P6" else 1
    return np.frombuffer(rest, np.uint8).reshape(int(h), int(w), cn)


def same32(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def test_demo_usage_names_the_flags(demo):  # noqa: F811
    r = subprocess.run([demo], capture_output=True, text=True)
    assert "--mask" in r.stderr and "--masked" in r.stderr and "--poses" in r.stderr


def test_demo_refuses_poses_without_camera_and_masked_without_mask(demo, tmp_path):  # noqa: F811
    mpath, ipath = _write_inputs(tmp_path, M.synthetic_tiny_model(thresh=0.7), synth.synthetic_frame(1, 96, 80, 3))
    r = subprocess.run([demo, mpath, ipath, "--poses"], capture_output=True, text=True)
    assert r.returncode != 0 and "--poses needs --depth and --camera" in r.stderr
    r = subprocess.run([demo, mpath, ipath, "--masked", str(tmp_path / "o.ppm")], capture_output=True, text=True)
    assert r.returncode != 0 and "--masked needs --mask" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--device-nms", "0.1"], ["--double", "--device-nms", "0.3", "--top", "4"]])
def test_demo_mask_and_poses_match_the_yardsticks(demo, tmp_path, flags):  # noqa: F811
    import torch
    torch.cuda.init()
    model = M.synthetic_person_model(thresh=17.9)
    im = synth.synthetic_frame(21, 160, 120, 3)
    mpath, ipath = _write_inputs(tmp_path, model, im)
    depth = synth.synthetic_depth(21, 160, 120, np.float32)
    dpath = tmp_path / "depth.pfm"
    dpath.write_bytes(b"Pf\n120 160\n-1.0\n" + np.ascontiguousarray(depth[::-1]).astype("<f4").tobytes())
    lab, out = tmp_path / "labels.pgm", tmp_path / "masked.ppm"
    r = subprocess.run([demo, mpath, ipath] + flags + ["--depth", str(dpath), "--camera", "600,590.5,59.5,80.25", "--poses", "--mask",
                                                       str(lab), "--masked", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, cands = _parse(r.stdout)
    assert cands
    cs = [Candidate(parts=parts, confidence=np.zeros(len(parts), np.float32), component=0) for _, _, parts in cands]
    want = Candidate.mask((160, 120), cs)
    got = read_pnm(lab)[:, :, 0]
    assert np.array_equal(got, want)
    assert int([ln for ln in r.stdout.splitlines() if ln.startswith("mask ")][0].split()[1]) == int((want != 0).sum())
    masked = read_pnm(out)[:, :, ::-1]                                       # PPM stores RGB; the demo's image is BGR
    assert np.array_equal(masked, publish.masked_image(im, want))
    _, centres, ncent, dense = PCC.computeBoundingBoxes(cs, [(160, 120)], [depth], [PinholeCamera(600.0, 590.5, 59.5, 80.25)])
    cnt, pos, quat, _ = publish.part_poses(centres, ncent, dense)
    pl = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("pose ")]
    assert len(pl) == len(cs)
    for i, t in enumerate(pl):
        assert int(t[0]) == cnt[i]
        assert same32([float(v) for v in t[1:4]], pos[i]) and same32([float(v) for v in t[4:8]], quat[i])
    assert (cnt > 0).any()


def test_bind_and_host_lines_compile(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('''
#include "pbd_host.hpp"
void use(pbdhost::PartsBasedDetector<float> &d, pbdhost::PartsBasedDetector<double> &e, const pbdhost::Image &im,
         const std::vector<pbdhost::Candidate> &c, const std::vector<std::vector<pbdhost::Point3f> > &centres,
         const std::vector<bool> &dense)
{
    std::vector<uint8_t> labels, masked;
    std::vector<int32_t> count;
    std::vector<float> pos, quat, ev;
    d.mask(im, c, labels);
    e.mask(im, c, labels, &masked);
    d.partPoses(centres, dense, count, pos, quat, ev);
    e.partPoses(centres, dense, count, pos, quat, ev);
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


TU = """#include "pbd_opencv_adapters.hpp"
template void pbd_adapters::hipCandidateMask<float>(pbd_handle *, const cv::Mat &, vectorCandidate &, cv::Mat &);
template void pbd_adapters::hipCandidateMask<double>(pbd_handle *, const cv::Mat &, vectorCandidate &, cv::Mat &);
template void pbd_adapters::hipPartPoses<float>(pbd_handle *, int, const std::vector<float> &, const std::vector<int32_t> &,
                                                const std::vector<int32_t> &, std::vector<int32_t> &, std::vector<float> &,
                                                std::vector<float> &, std::vector<float> &);
template void pbd_adapters::hipPartPoses<double>(pbd_handle *, int, const std::vector<float> &, const std::vector<int32_t> &,
                                                 const std::vector<int32_t> &, std::vector<int32_t> &, std::vector<float> &,
                                                 std::vector<float> &, std::vector<float> &);
"""


@pytest.mark.parametrize("std", ["c++98", "c++11", "c++17"])
def test_adapter_calls_compile_against_the_c_abi(std, tmp_path):
    src = tmp_path / "publish_tu.cpp"
    src.write_text(TU)
    cmd = ["g++", f"-std={std}", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", DOUBLES_DEPTH, "-I", DOUBLES, "-I",
           os.path.join(DOUBLES, "iface"), "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
