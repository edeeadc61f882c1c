"""ctypes binding of the C ABI in include/pbd.h (libpbd_hip.so).

Fails loudly when the library is missing or cannot be loaded: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBD_LIB", os.path.join(HERE, "libpbd_hip.so"))
MAX_LEVELS = 128

PBD_OK = 0
STATUS = {0: "PBD_OK", -1: "PBD_ERR_INVALID", -2: "PBD_ERR_UNSUPPORTED", -3: "PBD_ERR_HIP", -4: "PBD_ERR_CAPACITY",
          -5: "PBD_ERR_STATE", -6: "PBD_ERR_NOMEM"}
REAL_F32, REAL_F64 = 0, 1
CONV_EXACT, CONV_FMA, CONV_MFMA, CONV_MFMA_F16 = 0, 1, 2, 3
WALK_REFERENCE, WALK_ARGMAX = 0, 1   # pbd_set_walk
CONV_MFMA_F64 = 4          # fp64 matrix cores, REAL_F64 handles only (include/pbd.h)
CONV_MFMA_ANY = 5          # CONV_MFMA's arithmetic for every filter size 1..31 and mixed banks, REAL_F32 handles only
CONV_MFMA_F16_ANY = 6      # CONV_MFMA_F16's arithmetic and fp16 resident responses, likewise
STAGE_FEATURES, STAGE_RESPONSES, STAGE_ROOTV, STAGE_ROOTI = 0, 1, 2, 3
# options of pbd_debug_set_option (forced launch choices of one handle; not declared in include/pbd.h)
DT_LANE_SHIFT, DT_COOP, DT_COOP_G, DP_BUDGET_MB, GRID_NMS_LANES, HOG_TWO_PASS = 0, 1, 2, 3, 4, 5
GRID_NMS_WAVE_SZ = 7       # kGnWaveSz: k_grid_nms runs one lane per block below this sz, one wave per block from it on
# cv::Mat::depth() codes of the image depths HOGFeatures::pyramid accepts (src/HOGFeatures.cpp:136-146)
DEPTH_CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 2, np.dtype(np.float32): 5, np.dtype(np.float64): 6}
KERNELS = ["k_resize", "k_pyrdown", "k_hog_hist", "k_hog_feat", "k_conv", "k_dt_rows", "k_dt_cols", "k_dp_combine",
           "k_dp_root", "k_argmin", "k_camera_boxes", "k_cl_crop_count", "k_cl_crop_scan", "k_cl_crop_scatter", "k_cl_clear",
           "k_cl_grid_count", "k_cl_grid_scan", "k_cl_grid_scatter", "k_cl_hook", "k_cl_label", "k_cl_best", "k_cl_select", "k_cl_out",
           "k_dc_classify", "k_dc_select", "k_dc_compact", "k_mk_hull", "k_mk_tile", "k_part_poses",
           "k_ex_walk", "k_ex_gather", "k_qp_write", "k_qp_score", "k_qp_pass", "k_qp_lincomb",
           "k_qp_slots", "k_qp_norm", "k_qp_wraw", "k_qp_gather", "k_warp", "k_warp_emit",
           "k_ev_nms_select", "k_ev_nms_pairs", "k_ev_nms_greedy", "k_ev_nms_emit", "k_ev_best", "k_ev_pck", "k_ev_apk_rank",
           "k_ev_apk_close", "k_ev_apk_ap", "k_qp_hinge", "k_km_trials", "k_km_pick", "k_grid_nms", "k_top_k", "k_depth_prune"]
# the profile ids of pbd_max_marginals / pbd_marginal_poses*, which follow KERNELS' (PBD_K_MM_*: id = len(KERNELS) + index)
KERNELS_MM = ["k_mm_dt_rows", "k_mm_dt_cols", "k_mm_messages", "k_mm_context", "k_mm_down", "k_mm_decode"]
KERNELS_SCALE_NMS = ["k_scale_nms"]   # PBD_K_SCALE_NMS, after PBD_K_MM_DECODE
MM_VALUES, MM_DOWN, MM_PARENT_X, MM_PARENT_Y, MM_PARENT_K = 0, 1, 2, 3, 4   # pbd_get_marginals' selector
PARTS_LITERAL, PARTS_XY = 0, 1   # pbd_boxes3d_camera's sample loop (include/pbd.h)

# every symbol include/pbd.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "pbd_create", "pbd_destroy", "pbd_last_error", "pbd_version", "pbd_candidate_stride", "pbd_binsize",
    "pbd_pyramid_plan", "pbd_set_level_shard", "pbd_set_nms", "pbd_features_pyramid", "pbd_get_pyramid_image", "pbd_conv_set_filters", "pbd_conv_pdf",
    "pbd_num_ptr_slots", "pbd_ptr_slot", "pbd_dp_min", "pbd_dp_argmin", "pbd_detect", "pbd_detect_batch",
    "pbd_detect_batch_device", "pbd_detect_typed", "pbd_detect_batch_submit", "pbd_detect_batch_wait",
    "pbd_detect_batch_device_submit", "pbd_detect_batch_device_out", "pbd_argmin_device_out", "pbd_stream", "pbd_get_stage", "pbd_profile_enable", "pbd_profile_reset", "pbd_profile_read",
    "pbd_kernel_name", "pbd_synchronize", "pbd_detect_frames", "pbd_detect_frames_device", "pbd_detect_frames_device_out",
    "pbd_boxes3d", "pbd_boxes3d_device", "pbd_boxes3d_camera", "pbd_boxes3d_camera_device", "pbd_cluster_objects",
    "pbd_cluster_objects_device", "pbd_remove_planes", "pbd_remove_planes_device", "pbd_depth_consistency",
    "pbd_depth_consistency_device", "pbd_suppress", "pbd_suppress_device", "pbd_candidate_mask", "pbd_candidate_mask_device",
    "pbd_part_poses", "pbd_part_poses_device", "pbd_model_vector_len", "pbd_model_vector", "pbd_example_stride", "pbd_examples",
    "pbd_examples_device", "pbd_detect_latent", "pbd_qp_create", "pbd_qp_destroy", "pbd_qp_last_error", "pbd_qp_add",
    "pbd_qp_add_device", "pbd_qp_fix", "pbd_qp_prune", "pbd_qp_one", "pbd_qp_opt", "pbd_qp_weights", "pbd_qp_scores", "pbd_qp_state",
    "pbd_qp_entries", "pbd_set_model_vector", "pbd_set_model_vector_device", "pbd_set_thresh", "pbd_qp_apply",
    "pbd_warp_positives", "pbd_warp_positives_device", "pbd_part_nms", "pbd_part_nms_device", "pbd_best_overlap",
    "pbd_best_overlap_device", "pbd_eval_pck", "pbd_eval_pck_device", "pbd_eval_apk", "pbd_eval_apk_device",
    "pbd_set_walk", "pbd_qp_clear", "pbd_qp_add_loss_device", "pbd_cluster_parts", "pbd_cluster_parts_device",
    "pbd_grid_nms", "pbd_grid_nms_device", "pbd_set_root_nms",
    "pbd_top_k_cells", "pbd_top_k_cells_device", "pbd_set_top_k", "pbd_top_k", "pbd_top_k_device",
    "pbd_set_depth_prune", "pbd_bind_depth", "pbd_bind_depth_device", "pbd_depth_prune", "pbd_depth_prune_device",
    "pbd_augment_plan", "pbd_augment_points", "pbd_augment_frames", "pbd_augment_frames_device", "pbd_detect_latent_device",
    "pbd_part_scores", "pbd_part_scores_device", "pbd_score_placements", "pbd_score_placements_device",
    "pbd_max_marginals", "pbd_get_marginals", "pbd_marginals_device", "pbd_marginal_poses", "pbd_marginal_poses_device",
    "pbd_set_padding", "pbd_set_fine_octave",
    "pbd_set_scale_nms", "pbd_scale_nms", "pbd_scale_nms_device",
]


class PbdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class CModel(C.Structure):
    _fields_ = [
        ("ncomponents", C.c_int), ("nfilters", C.c_int), ("flen", C.c_int),
        ("filter_ksize", C.POINTER(C.c_int)), ("filter_offset", C.POINTER(C.c_int64)),
        ("filters_f32", C.POINTER(C.c_float)), ("filters_f64", C.POINTER(C.c_double)),
        ("nbias", C.c_int), ("biasw", C.POINTER(C.c_float)),
        ("ndefs", C.c_int), ("defw", C.POINTER(C.c_float)), ("anchors", C.POINTER(C.c_int)),
        ("part_offset", C.POINTER(C.c_int)), ("parentid", C.POINTER(C.c_int)),
        ("mix_offset", C.POINTER(C.c_int)), ("filterid", C.POINTER(C.c_int)),
        ("biasid", C.POINTER(C.c_int)), ("defid", C.POINTER(C.c_int)),
        ("thresh", C.c_float), ("sbin", C.c_int), ("interval", C.c_int), ("norient", C.c_int),
    ]


class CFrame(C.Structure):
    """pbd_frame: one frame of a mixed-size call (host pointer, or device pointer for the _device forms)."""
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("stride_bytes", C.c_size_t)]


class CAugment(C.Structure):
    """pbd_augment: one copy of a call: the frame's index, mirror (0 / 1), degrees (counter-clockwise)"""
    _fields_ = [("frame", C.c_int32), ("mirror", C.c_int32), ("degrees", C.c_double)]


def augment_array(jobs):
    """(pbd_augment[]) from (frame, mirror, degrees) tuples"""
    arr = (CAugment * len(jobs))()
    for i, (f, m, d) in enumerate(jobs):
        arr[i].frame, arr[i].mirror, arr[i].degrees = int(f), 1 if m else 0, float(d)
    return arr


class CDepthPruneCfg(C.Structure):
    """pbd_depth_prune_cfg: focal length in pixels, the root footprint's physical width in depth units, relative tolerance"""
    _fields_ = [("fx", C.c_float), ("width", C.c_float), ("tol", C.c_float)]


def prune_cfg(fx: float, width: float, tol: float):
    """(const pbd_depth_prune_cfg *) of the three values"""
    return C.byref(CDepthPruneCfg(float(fx), float(width), float(tol)))


class CPinhole(C.Structure):
    """pbd_pinhole: one frame's pinhole intrinsics"""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "tx", "ty")]


class CCloud(C.Structure):
    """pbd_cloud: one point cloud (x, y, z the first three floats of every point)"""
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("point_stride", C.c_size_t), ("row_stride", C.c_size_t)]


class CPlaneParams(C.Structure):
    """pbd_plane_params (pointcloud.PlaneParams)"""
    _fields_ = [("smoothing_size", C.c_int), ("depth_change_factor", C.c_float), ("distance_threshold", C.c_float),
                ("angular_threshold", C.c_double), ("max_curvature", C.c_double), ("min_inliers", C.c_int), ("refine", C.c_int)]


def plane_params(q):
    """a CPlaneParams from an object with PlaneParams' fields, or None (the reference's call)"""
    if q is None:
        return None
    out = CPlaneParams()
    for name, _ in CPlaneParams._fields_:
        setattr(out, name, getattr(q, name))
    return C.pointer(out)


def pinhole_array(cams):
    """(pbd_pinhole[]) from objects with fx, fy, cx, cy, tx, ty"""
    arr = (CPinhole * len(cams))()
    for i, c in enumerate(cams):
        for k in ("fx", "fy", "cx", "cy", "tx", "ty"):
            setattr(arr[i], k, float(getattr(c, k)))
    return arr


def cloud_array(descs):
    """(pbd_cloud[]) from (pointer, rows, cols, point_stride, row_stride) tuples"""
    arr = (CCloud * len(descs))()
    for i, (p, r, c, ps, rs) in enumerate(descs):
        arr[i].data, arr[i].rows, arr[i].cols, arr[i].point_stride, arr[i].row_stride = p, r, c, ps, rs
    return arr


def frame_array(descs):
    """(pbd_frame[]) from (pointer, rows, cols, stride_bytes) tuples."""
    arr = (CFrame * len(descs))()
    for i, (p, r, c, st) in enumerate(descs):
        arr[i].data, arr[i].rows, arr[i].cols, arr[i].stride_bytes = p, r, c, st
    return arr


# ---- marshalling rules of the Python binding, each stated once ------------------------------------------------------------
def opt_ptr(a):
    """the address of an array's data, or None for an empty array"""
    return a.ctypes.data if a.size else None


def real_code(dtype) -> int:
    """REAL_F32 / REAL_F64 of a float dtype"""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise PbdError(-1, f"dtype {dt}: float32 or float64")
    return REAL_F32 if dt == np.float32 else REAL_F64


def shape_arrays(im_shapes):
    """(rows, cols, their POINTER(c_int)s) of im_shapes[f] = (rows, cols), as int32 arrays; a pointer keeps its array alive"""
    ir = np.array([int(s[0]) for s in im_shapes], np.int32)
    ic = np.array([int(s[1]) for s in im_shapes], np.int32)
    return ir, ic, ptr(ir, C.c_int), ptr(ic, C.c_int)


def depth_frames(depths):
    """(arrays kept alive, pbd_frame[], depth code) of 2-D depth images of one dtype, rows of any pitch"""
    dt = np.dtype(depths[0].dtype)
    if dt not in DEPTH_CODE or any(np.dtype(d.dtype) != dt for d in depths):
        raise PbdError(-1, "one depth dtype per call: uint8, uint16, float32 or float64")
    ds = [d if d.ndim == 2 and d.strides[1] == d.itemsize and d.strides[0] > 0 else np.ascontiguousarray(d) for d in depths]
    return ds, frame_array([(d.ctypes.data, d.shape[0], d.shape[1], d.strides[0]) for d in ds]), DEPTH_CODE[dt]


def hwc(f):
    """rows x cols x channels of an image given as rows x cols or rows x cols x channels (a view)"""
    return f if f.ndim == 3 else f[:, :, None]


def image_frames(frames, bad_dtype: int = -1):
    """(arrays kept alive, pbd_frame[], channels, depth code) of HW or HWC images of any sizes, of one dtype of DEPTH_CODE's four
    (another one: PbdError(bad_dtype)) and one channel count.  A frame whose pixels are contiguous -- channels `itemsize` apart
    (one channel: wherever), pixels `cn * itemsize` apart, a positive row pitch -- is described in place with that pitch, a
    region of a larger image included; any other frame gets one contiguous copy.  No frames: 3 channels, code 0."""
    fr = [hwc(f) for f in frames]
    if not fr:
        return fr, frame_array([]), 3, 0
    dt, cn = fr[0].dtype, fr[0].shape[2]
    if any(f.dtype != dt for f in fr):
        raise PbdError(-1, "one call takes one image dtype: " + ", ".join(sorted({str(f.dtype) for f in fr})))
    if dt not in DEPTH_CODE:
        raise PbdError(bad_dtype, f"image dtype {dt}: uint8, uint16, float32 or float64 (src/HOGFeatures.cpp:136-146)")
    if any(f.shape[2] != cn for f in fr):
        raise PbdError(-1, "one call takes one channel count: " + ", ".join(sorted({str(f.shape[2]) for f in fr})))
    es = dt.itemsize
    fr = [f if (cn == 1 or f.strides[2] == es) and f.strides[1] == cn * es and f.strides[0] > 0 else np.ascontiguousarray(f) for f in fr]
    return fr, frame_array([(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0]) for f in fr]), cn, DEPTH_CODE[dt]


def pack_arrays(arrays, masks, name: str):
    """(arrays, real code, packed values, packed mask bytes or None) of float arrays of one dtype, any shapes, empty ones included,
    and of None or one uint8 / bool mask of its array's shape per array: values and masks (non-zero -> 1) concatenated in order"""
    arrs = [np.ascontiguousarray(a) for a in arrays]
    dt = arrs[0].dtype if arrs else np.dtype(np.float32)
    if dt not in (np.float32, np.float64) or any(a.dtype != dt for a in arrs):
        raise PbdError(-1, f"{name}: arrays of one dtype, float32 or float64")
    if masks is not None and (len(masks) != len(arrs) or any(np.shape(m) != a.shape for m, a in zip(masks, arrs))):
        raise PbdError(-1, f"{name}: one mask of its array's shape per array")
    src = np.concatenate([a.ravel() for a in arrs] or [np.zeros(0, dt)])
    msk = None if masks is None else np.concatenate([(np.asarray(m) != 0).astype(np.uint8).ravel() for m in masks] or [np.zeros(0, np.uint8)])
    return arrs, real_code(dt), src, msk


def split_arrays(packed, arrays):
    """pack_arrays' inverse on a packed per-element result: one array per input array, in its shape"""
    off = np.concatenate([[0], np.cumsum([a.size for a in arrays], dtype=np.int64)])
    return [packed[off[i]:off[i + 1]].reshape(a.shape) for i, a in enumerate(arrays)]


class CQpConfig(C.Structure):
    _fields_ = [("capacity", C.c_int), ("C", C.c_double), ("wpos", C.c_double), ("stream", C.c_void_p), ("wreg", C.c_void_p),
                ("w0", C.c_void_p), ("noneg", C.c_void_p), ("nnoneg", C.c_int)]


class CQpInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n", "nsv", "nfix", "capacity", "len", "hdr_words", "values")] + \
               [(n, C.c_double) for n in ("lb", "ub", "loss", "l")] + [(n, C.c_int) for n in ("lb_dropped", "passes", "converged", "pad")]


class CClusterInfo(C.Structure):
    """pbd_cluster_info: the picked trial of one part"""
    _fields_ = [("best_trial", C.c_int32), ("iterations", C.c_int32), ("sumdist", C.c_double)]


CLUSTER_INFO_DTYPE = np.dtype([("best_trial", np.int32), ("iterations", np.int32), ("sumdist", np.float64)])
MAX_MIX = 16               # kMaxMix: types per part; a row of pbd_cluster_parts' centres, counts and anchors
KM_MAX_GRID = 2048         # workgroups of k_km_trials; more (part, trial) pairs are taken in a stride loop


class CConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("real_type", C.c_int), ("conv_mode", C.c_int), ("max_batch", C.c_int),
                ("max_candidates", C.c_int), ("stream", C.c_void_p)]


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


_LIB = None


def load():
    """Load libpbd_hip.so (building it first is __graft_entry__.build()'s job)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -m partsbaseddetector_amd.build` "
                          "(the HIP extension is required; there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.pbd_last_error.restype = C.c_char_p
    lib.pbd_last_error.argtypes = [C.c_void_p]
    lib.pbd_version.restype = C.c_char_p
    lib.pbd_kernel_name.restype = C.c_char_p
    lib.pbd_create.argtypes = [C.POINTER(CModel), C.POINTER(CConfig), C.POINTER(C.c_void_p)]
    lib.pbd_destroy.argtypes = [C.c_void_p]
    lib.pbd_destroy.restype = None
    for name in ("pbd_candidate_stride", "pbd_binsize", "pbd_num_ptr_slots", "pbd_synchronize", "pbd_profile_reset"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.pbd_ptr_slot.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pbd_set_level_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pbd_set_nms.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.pbd_set_walk.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_set_padding.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pbd_set_fine_octave.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_set_root_nms.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_grid_nms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p]
    lib.pbd_grid_nms_device.argtypes = lib.pbd_grid_nms.argtypes
    lib.pbd_debug_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pbd_debug_postprocess.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                          C.POINTER(C.c_int)]
    lib.pbd_pyramid_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_float)]
    lib.pbd_features_pyramid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                         C.POINTER(C.c_void_p)]
    lib.pbd_get_pyramid_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pbd_conv_set_filters.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    lib.pbd_conv_pdf.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_void_p)]
    lib.pbd_dp_min.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_void_p)] * 6
    lib.pbd_dp_argmin.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                               C.POINTER(C.c_int)]
    lib.pbd_detect_typed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_int,
                                     C.POINTER(C.c_int)]
    lib.pbd_detect_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_size_t,
                                     C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_detect_batch_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_size_t]
    lib.pbd_detect_batch_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_detect_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_int, C.POINTER(C.c_int)]
    lib.pbd_detect_batch_device_submit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.pbd_detect_batch_device_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.pbd_argmin_device_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.pbd_detect_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_detect_frames_device.argtypes = lib.pbd_detect_frames.argtypes
    lib.pbd_detect_frames_device_out.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_int]
    lib.pbd_boxes3d.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                C.c_int, C.c_int, C.c_void_p]
    lib.pbd_boxes3d_device.argtypes = lib.pbd_boxes3d.argtypes
    lib.pbd_boxes3d_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(CPinhole), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
    lib.pbd_boxes3d_camera_device.argtypes = lib.pbd_boxes3d_camera.argtypes
    lib.pbd_cluster_objects.argtypes = [C.c_void_p, C.c_int, C.POINTER(CCloud), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_cluster_objects_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(CCloud), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_remove_planes.argtypes = [C.c_void_p, C.c_int, C.POINTER(CCloud), C.POINTER(CPlaneParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_remove_planes_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(CCloud), C.POINTER(CPlaneParams), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.pbd_depth_consistency.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_depth_consistency_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_float, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_int]
    lib.pbd_set_top_k.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_top_k_cells.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.pbd_top_k_cells_device.argtypes = lib.pbd_top_k_cells.argtypes
    lib.pbd_top_k.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_top_k_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.pbd_set_scale_nms.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pbd_scale_nms.argtypes = lib.pbd_top_k.argtypes
    lib.pbd_scale_nms_device.argtypes = lib.pbd_top_k_device.argtypes
    lib.pbd_set_depth_prune.argtypes = [C.c_void_p, C.POINTER(CDepthPruneCfg)]
    lib.pbd_bind_depth.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int]
    lib.pbd_bind_depth_device.argtypes = lib.pbd_bind_depth.argtypes
    lib.pbd_depth_prune.argtypes = [C.c_void_p, C.POINTER(CDepthPruneCfg), C.c_int, C.POINTER(CFrame), C.c_int, C.c_void_p, C.c_int,
                                    C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_depth_prune_device.argtypes = [C.c_void_p, C.POINTER(CDepthPruneCfg), C.c_int, C.POINTER(CFrame), C.c_int, C.c_void_p,
                                           C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.pbd_suppress.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.pbd_suppress_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int]
    lib.pbd_candidate_mask.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_candidate_mask_device.argtypes = lib.pbd_candidate_mask.argtypes + [C.c_void_p]
    lib.pbd_part_poses.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lib.pbd_part_poses_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lib.pbd_model_vector_len.argtypes = [C.c_void_p]
    lib.pbd_model_vector.argtypes = [C.c_void_p, C.c_void_p]
    lib.pbd_set_model_vector.argtypes = [C.c_void_p, C.c_void_p]
    lib.pbd_set_model_vector_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.pbd_set_thresh.argtypes = [C.c_void_p, C.c_float]
    lib.pbd_qp_apply.argtypes = [C.c_void_p, C.c_void_p]
    lib.pbd_example_stride.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pbd_examples.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pbd_examples_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for fn in (lib.pbd_part_scores, lib.pbd_part_scores_device, lib.pbd_score_placements, lib.pbd_score_placements_device):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_max_marginals.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_get_marginals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.pbd_marginals_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.pbd_marginal_poses.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_marginal_poses_device.argtypes = lib.pbd_marginal_poses.argtypes
    lib.pbd_warp_positives.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_warp_positives_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pbd_part_nms.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_int)]
    lib.pbd_part_nms_device.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.pbd_best_overlap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pbd_best_overlap_device.argtypes = lib.pbd_best_overlap.argtypes
    lib.pbd_eval_pck.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.pbd_eval_pck_device.argtypes = lib.pbd_eval_pck.argtypes
    lib.pbd_eval_apk.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_eval_apk_device.argtypes = lib.pbd_eval_apk.argtypes + [C.c_void_p]
    lib.pbd_detect_latent.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                      C.c_void_p, C.c_void_p]
    lib.pbd_detect_latent_device.argtypes = lib.pbd_detect_latent.argtypes
    lib.pbd_augment_plan.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.pbd_augment_points.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pbd_augment_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFrame), C.c_int, C.c_int, C.c_int, C.POINTER(CAugment),
                                       C.POINTER(CFrame)]
    lib.pbd_augment_frames_device.argtypes = lib.pbd_augment_frames.argtypes
    lib.pbd_qp_create.argtypes = [C.c_void_p, C.POINTER(CQpConfig), C.POINTER(C.c_void_p)]
    lib.pbd_qp_destroy.argtypes = [C.c_void_p]
    lib.pbd_qp_destroy.restype = None
    lib.pbd_qp_last_error.argtypes = [C.c_void_p]
    lib.pbd_qp_last_error.restype = C.c_char_p
    lib.pbd_qp_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.pbd_qp_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p]
    lib.pbd_qp_fix.argtypes = [C.c_void_p]
    lib.pbd_qp_clear.argtypes = [C.c_void_p]
    lib.pbd_qp_add_loss_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.pbd_qp_prune.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.pbd_qp_one.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(CQpInfo)]
    lib.pbd_qp_opt.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint64, C.POINTER(CQpInfo)]
    lib.pbd_qp_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.pbd_qp_scores.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.pbd_qp_state.argtypes = [C.c_void_p, C.POINTER(CQpInfo), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pbd_qp_entries.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.pbd_cluster_parts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64] + \
                                     [C.c_void_p] * 7
    lib.pbd_cluster_parts_device.argtypes = lib.pbd_cluster_parts.argtypes
    lib.pbd_debug_mixed_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.c_int]
    lib.pbd_stream.argtypes = [C.c_void_p]
    lib.pbd_stream.restype = C.c_void_p
    lib.pbd_get_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.pbd_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.pbd_profile_read.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.pbd_kernel_name.argtypes = [C.c_int]
    _LIB = lib
    return lib


def c_model(flat) -> CModel:
    m = CModel()
    m.ncomponents, m.nfilters, m.flen = flat.ncomponents, flat.nfilters, flat.flen
    m.filter_ksize = ptr(flat.filter_ksize, C.c_int)
    m.filter_offset = ptr(flat.filter_offset, C.c_int64)
    m.filters_f32 = ptr(flat.filters_f32, C.c_float)
    m.filters_f64 = ptr(flat.filters_f64, C.c_double)
    m.nbias, m.biasw = len(flat.biasw), ptr(flat.biasw, C.c_float)
    m.ndefs, m.defw, m.anchors = len(flat.defw), ptr(flat.defw, C.c_float), ptr(flat.anchors, C.c_int)
    m.part_offset, m.parentid = ptr(flat.part_offset, C.c_int), ptr(flat.parentid, C.c_int)
    m.mix_offset, m.filterid = ptr(flat.mix_offset, C.c_int), ptr(flat.filterid, C.c_int)
    m.biasid, m.defid = ptr(flat.biasid, C.c_int), ptr(flat.defid, C.c_int)
    m.thresh, m.sbin, m.interval, m.norient = flat.thresh, flat.sbin, flat.interval, flat.norient
    m._keep = flat
    return m


def ptr_array(arrays):
    """(void*[]) over a list of numpy arrays; returns (ctypes array, keepalive)."""
    arr = (C.c_void_p * len(arrays))()
    for i, a in enumerate(arrays):
        arr[i] = a.ctypes.data if a is not None and a.size else None
    return arr
