"""Plane removal and object clustering on the device against the built hard clouds of tests/cloud_hard_scenes.py: every kernel of
pbd_kernels_planes.hip and pbd_kernels_cloud.hip on the branches no smooth scene reaches ("Built hard clouds" has the table).

The yardstick is partsbaseddetector_amd/pointcloud.py (pinned on these scenes by tests/test_cloud_hard_cpu.py).  Every comparison
is exact: BIT PATTERNS for points, plane coefficients and centres; labels, counts, kept lists and index lists as integers.  There
is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import cloud_hard_scenes as S
from partsbaseddetector_amd import detector
from partsbaseddetector_amd import model as M
from partsbaseddetector_amd.detector import PbdError
from partsbaseddetector_amd.pointcloud import PointCloudClusterer as PCC

pytestmark = pytest.mark.gpu

PLANE_CALLS = {"joins": ["cos_equal", "dist_equal", "depth_step"],
               "tall": ["4097x13", "4100x24", "small_4100_4097", "1024x16_1025x16"],
               "snake": ["snake", "snake_T", "comb"],
               "singles": ["checker_70x70", "patches_15x15"],
               "far": ["far"],
               "edges": ["around_2s+3", "collinear", "ballot_tiles", "moment_rounds", "special_values", "flat_1023", "checker_1023",
                         "flat_1024", "checker_1024", "flat_1025", "checker_1025", "flat_2049", "checker_2049", "flat_2048",
                         "checker_2048", "flat_2049T", "checker_2049T"],
               "refine": ["upper_right_nan", "upper_right_finite", "last_column", "last_row", "upper_beats_left", "staircase",
                          "thresholds"],
               "many": ["many"]}
CLUSTER_CALLS = {"chain": ["shuffled", "reversed", "even_odd"],
                 "faces": ["faces"],
                 "dense": ["dense"],
                 "ties": ["2x2", "3x2", "2x300", "3x300", "301_300_301"],
                 "boxes": ["300", "4200", "crop_1", "crop_2", "crop_3", "on_faces", "crop_2_x40"],
                 "chunks": ["1023", "1024", "1025", "2049", "5000_and_60", "5_floats_padded"]}
PLANE_IDS = [(f, n) for f, names in PLANE_CALLS.items() for n in names]
CLUSTER_IDS = [(f, n) for f, names in CLUSTER_CALLS.items() for n in names]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def hd():
    h = detector.Handle(M.synthetic_person_model(), device=0, max_batch=2)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def plane_calls(family):
    return S.PLANE_SCENES[family]()


@functools.lru_cache(maxsize=None)
def cluster_calls(family):
    return S.CLUSTER_SCENES[family]()


@functools.lru_cache(maxsize=None)
def plane_want(family, name):
    """per cloud: (points, kept, labels, planes, inliers) of its single-cloud yardstick; computed once, never modified"""
    call = plane_calls(family)[name]
    out = []
    with np.errstate(all="ignore"):
        for c in call.clouds:
            pts, kept, labels, planes = PCC.organizedMultiplaneSegmentation(c, call.params)
            out.append((pts, kept, labels, planes, np.bincount(labels[labels >= 0], minlength=len(planes)).astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def cluster_want(family, name):
    call = cluster_calls(family)[name]
    return PCC.clusterObjects(call.clouds, call.boxes, call.frames)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def assert_planes_same(got, want):
    pts, kept, labels, planes, inl = got
    wp, wk, wl, wpl, wi = want
    assert np.array_equal(labels, wl), np.argwhere(labels != wl)[:5]
    assert np.array_equal(bits(planes), bits(wpl)), (planes[:3], wpl[:3])
    assert np.array_equal(inl, wi)
    assert np.array_equal(kept, wk)
    assert np.array_equal(bits(pts), bits(wp))


def assert_clusters_same(got, want):
    cen, cnt, idx = got
    wc, wi = want
    assert bits(cen).shape == bits(wc).shape and np.array_equal(bits(cen), bits(wc)), np.nonzero((bits(cen) != bits(wc)).any(axis=1))[0][:5]
    assert list(cnt) == [len(v) for v in wi]
    assert np.array_equal(idx, np.concatenate(list(wi) + [np.zeros(0, np.int64)]))


# ---- every scene through the host forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name", PLANE_IDS)
def test_plane_scene_bit_exact(hd, family, name):
    call = plane_calls(family)[name]
    got = hd.remove_planes(call.clouds, call.params)
    assert len(got) == len(call.clouds)
    for g, w in zip(got, plane_want(family, name)):
        assert_planes_same(g, w)


def test_plane_capacity_below_at_and_above_the_count(hd):
    call = plane_calls("singles")["patches_15x15"]
    (want,) = plane_want("singles", "patches_15x15")
    n = len(want[3])
    assert n == 225
    with pytest.raises(PbdError) as e:
        hd.remove_planes(call.clouds, call.params, plane_capacity=n - 1)
    assert e.value.code == -4 and e.value.needed == n
    for cap in (n, n + 75):
        (got,) = hd.remove_planes(call.clouds, call.params, plane_capacity=cap)
        assert_planes_same(got, want)


@pytest.mark.parametrize("family,name", CLUSTER_IDS)
def test_cluster_scene_bit_exact(hd, family, name):
    call = cluster_calls(family)[name]
    assert_clusters_same(hd.cluster_objects(call.clouds, call.boxes, call.frames), cluster_want(family, name))


@pytest.mark.parametrize("total", [S.HOST_CROP - 1, S.HOST_CROP, S.HOST_CROP + 1])
def test_crop_edge_first_on_a_fresh_handle_then_again(total):
    """the host form's first crop capacity is max(what the handle has needed so far, 65536): 65537 cropped points take the second
    pass on a fresh handle and the first on the same handle afterwards"""
    call = S.crop_edge()[str(total)]
    want = PCC.clusterObjects(call.clouds, call.boxes, call.frames)
    assert len(want[1][0]) == total
    h = detector.Handle(M.synthetic_person_model(), device=0, max_batch=2)
    try:
        first = h.cluster_objects(call.clouds, call.boxes, call.frames)
        again = h.cluster_objects(call.clouds, call.boxes, call.frames)
    finally:
        h.close()
    assert_clusters_same(first, want)
    assert_clusters_same(again, want)
    for a, b in zip(first, again):
        assert np.array_equal(np.asarray(a).view(np.uint32) if a.dtype == np.float32 else a,
                              np.asarray(b).view(np.uint32) if b.dtype == np.float32 else b)


# ---- the device forms ---------------------------------------------------------------------------------------------------------
GUARD = -77


def region(torch, cloud, k, fill):
    """the cloud as a region of a larger device buffer: point stride 16 or 20 bytes, rows padded by `k + 1` points, two rows and
    three columns of `fill` around it; returns (buffer, descriptor)"""
    c = np.asarray(cloud)
    if c.ndim == 2:
        c = c[None]
    rows, cols = c.shape[:2]
    floats = 4 + k % 2
    big = torch.full((rows + 4, cols + 6 + k + 1, floats), fill, dtype=torch.float32, device="cuda")
    big[2:2 + rows, 3:3 + cols, :3] = torch.from_numpy(np.ascontiguousarray(c[:, :, :3])).cuda()
    return big, (big[2, 3].data_ptr(), rows, cols, 4 * floats, big.shape[1] * 4 * floats)


@pytest.mark.parametrize("family,name", [("tall", "small_4100_4097"), ("tall", "1024x16_1025x16"), ("many", "many")])
def test_planes_device_form_regions_strides_and_guards(hd, family, name):
    import torch
    call = plane_calls(family)[name]
    wants = plane_want(family, name)
    keep = [region(torch, c, k, 7.0) for k, c in enumerate(call.clouds)]
    descs = [d for _, d in keep]
    sizes = [c.shape[0] * c.shape[1] for c in call.clouds]
    nc, total = len(sizes), sum(sizes)
    most = max(len(w[3]) for w in wants)
    for cap in (most, max(most - 1, 1)):
        pts = torch.full((total + 1, 3), 5.0, dtype=torch.float32, device="cuda")
        kept = torch.full((total + 1,), GUARD, dtype=torch.int32, device="cuda")
        lab = torch.full((total + 1,), GUARD, dtype=torch.int32, device="cuda")
        nk = torch.full((nc + 1,), GUARD, dtype=torch.int32, device="cuda")
        npl = torch.full((nc + 1,), GUARD, dtype=torch.int32, device="cuda")
        pl = torch.full((nc * cap + 1, 4), 9.0, dtype=torch.float32, device="cuda")
        inl = torch.full((nc * cap + 1,), GUARD, dtype=torch.int32, device="cuda")
        st = torch.full((3,), GUARD, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hd.remove_planes_device(descs, call.params, pts.data_ptr(), kept.data_ptr(), nk.data_ptr(), lab.data_ptr(), pl.data_ptr(),
                                inl.data_ptr(), npl.data_ptr(), cap, st.data_ptr())
        torch.cuda.synchronize()
        pts, kept, nk, lab = pts.cpu().numpy(), kept.cpu().numpy(), nk.cpu().numpy(), lab.cpu().numpy()
        pl, inl, npl, st = pl.cpu().numpy(), inl.cpu().numpy(), npl.cpu().numpy(), st.cpu().numpy()
        base = 0
        for i, (wp, wk, wl, wpl, wi) in enumerate(wants):
            n, k = sizes[i], len(wk)
            assert nk[i] == k and npl[i] == len(wpl), i
            assert np.array_equal(lab[base:base + n].reshape(wl.shape), wl), i
            assert np.array_equal(kept[base:base + k], wk) and (kept[base + k:base + n] == -1).all()
            assert np.array_equal(bits(pts[base:base + k]), bits(wp)) and np.isnan(pts[base + k:base + n]).all()
            w = min(len(wpl), cap)
            assert np.array_equal(bits(pl[i * cap:i * cap + w]), bits(wpl[:w]))
            assert np.array_equal(inl[i * cap:i * cap + w], wi[:w])
            assert (inl[i * cap + w:(i + 1) * cap] == GUARD).all() and (pl[i * cap + w:(i + 1) * cap] == 9.0).all()
            base += n
        assert (pts[total] == 5.0).all() and kept[total] == GUARD and lab[total] == GUARD and nk[nc] == GUARD and npl[nc] == GUARD
        assert (pl[nc * cap] == 9.0).all() and inl[nc * cap] == GUARD and st[2] == GUARD
        assert st[0] == nk[:nc].sum() and st[1] == most
    for big, _ in keep:                               # the clouds' surroundings were only read
        assert (big[0] == 7.0).all() and (big[:, :3] == 7.0).all() and (big[..., 3:] == 7.0).all()


@pytest.mark.parametrize("family,name", [("boxes", "300"), ("boxes", "4200"), ("boxes", "crop_2_x40"), ("chunks", "2049"),
                                         ("chunks", "5000_and_60"), ("chunks", "5_floats_padded")])
def test_clusters_device_form_regions_payload_frames_and_capacities(hd, family, name):
    import torch
    call = cluster_calls(family)[name]
    wc, wi = cluster_want(family, name)
    nan = float("nan")
    keep = [region(torch, c, k, nan) for k, c in enumerate(call.clouds)]
    descs = [d for _, d in keep]
    n = len(call.boxes)
    offset = 5
    # two more records than boxes of the call: one of a frame before the call's, one of a frame after it; the payload claims
    # seven more records than the capacity holds
    outside = [0, n + 1]
    rec = np.zeros((n + 2, hd.stride), np.int32)
    rec[1:n + 1, 0] = np.asarray(call.frames) + offset
    rec[0, 0] = offset - 1
    rec[n + 1, 0] = offset + len(call.clouds)
    cap = n + 2
    pay = torch.from_numpy(np.concatenate([[cap + 7], rec.ravel()]).astype(np.int32)).cuda()
    boxes = np.concatenate([call.boxes[:1], call.boxes, call.boxes[:1]])
    bx = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).cuda()
    total = sum(len(v) for v in wi)
    want_idx = np.concatenate(list(wi) + [np.zeros(0, np.int64)])
    cropped = None
    for index_cap in (total, total - 1):
        if index_cap < 0:
            continue
        oc = torch.full((cap + 1, 3), 9.0, dtype=torch.float32, device="cuda")
        cn = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
        ix = torch.full((total + 64,), GUARD, dtype=torch.int32, device="cuda")
        st = torch.full((3,), GUARD, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hd.cluster_objects_device(descs, pay.data_ptr(), cap, offset, bx.data_ptr(), 1 << 20, index_cap, oc.data_ptr(), cn.data_ptr(),
                                  ix.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
        s, o, c, i = st.cpu().numpy(), oc.cpu().numpy(), cn.cpu().numpy(), ix.cpu().numpy()
        assert (o[cap] == 9.0).all() and c[cap] == GUARD and s[2] == GUARD
        assert s[1] == total and s[0] >= total
        cropped = s[0] if cropped is None else cropped
        assert s[0] == cropped
        for k in outside:                             # a box whose frame is outside the call crops nothing
            assert c[k] == 0 and np.isnan(o[k]).all()
        assert np.array_equal(bits(o[1:n + 1]), bits(wc)) and list(c[1:n + 1]) == [len(v) for v in wi]
        if index_cap == total:
            assert np.array_equal(i[:total], want_idx) and (i[total:] == GUARD).all()
        else:
            assert (i == GUARD).all()                 # one index short: nothing is written, status[1] says how many
    for big, _ in keep:
        assert torch.isnan(big[0]).all() and torch.isnan(big[..., 3:]).all()
