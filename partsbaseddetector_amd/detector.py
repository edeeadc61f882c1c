"""Host-side mirror of the reference's operator interface for the detection hot path, over the
C ABI (include/pbd.h).  Same names and argument meaning as the reference:

    IFeatures / HOGFeatures<T>            include/IFeatures.hpp:49-73, src/HOGFeatures.cpp
    IConvolutionEngine / Spatial...       include/IConvolutionEngine.hpp:44-68, src/SpatialConvolutionEngine.cpp
    DynamicProgram<T>                     include/DynamicProgram.hpp:74-75, src/DynamicProgram.cpp
    PartsBasedDetector<T>                 include/PartsBasedDetector.hpp:152-175, src/PartsBasedDetector.cpp
    Candidate                             include/Candidate.hpp:56-216

Every compute call runs HIP kernels through libpbd_hip.so; nothing here computes on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import PbdError
from .model import FlatModel, Model


@dataclass
class Candidate:
    """include/Candidate.hpp:56-80: part rectangles (x, y, w, h), confidences, component.
    `frame`, `level`, `root` record where the candidate was back-tracked from."""

    parts: np.ndarray
    confidence: np.ndarray
    component: int
    frame: int = 0
    level: int = 0
    root: tuple = (0, 0)
    offset: tuple = (0, 0)   # (x, y) of the region the candidate was found in (detect_regions); boxes are region-relative
    mixtures: np.ndarray = None   # the type (mixture) of every part, set by PartsBasedDetector.partScores
    place: np.ndarray = None      # the cell (x, y) of every part in its level's map, set by PartsBasedDetector.marginalPoses

    def score(self) -> float:  # Candidate.hpp:82
        return float(self.confidence[0]) if len(self.confidence) else float("-inf")

    @staticmethod
    def sort(candidates: List["Candidate"]) -> None:  # Candidate.hpp:91-99 (descending by score)
        candidates.sort(key=lambda c: -c.score())

    def boundingBox(self):
        """Candidate.hpp:105-111: hull of the part rectangles (cv::Rect operator|), as (x, y, w, h)."""
        x, y, w, h = (int(v) for v in self.parts[0])
        for r in self.parts:
            bx, by, bw, bh = (int(v) for v in r)
            if w <= 0 or h <= 0:            # a.empty(): a = b
                x, y, w, h = bx, by, bw, bh
            elif bw > 0 and bh > 0:
                x1, y1 = min(x, bx), min(y, by)
                w, h = max(x + w, bx + bw) - x1, max(y + h, by + bh) - y1
                x, y = x1, y1
        return x, y, w, h

    def boundingBoxNorm(self):
        """Candidate.hpp:117-130: Rect(mean - 1.5 std, 3 std) of the part centroids, as (x, y, w, h).  A centroid is
        cvRound((tl + br) * 0.5) (half to even); cv::meanStdDev sums in double; the double -> int conversions truncate."""
        s = [0.0, 0.0]
        sq = [0.0, 0.0]
        for x, y, w, h in (tuple(int(v) for v in r) for r in self.parts):
            for c, v in enumerate((float(round((2 * x + w) * 0.5)), float(round((2 * y + h) * 0.5)))):
                s[c] += v
                sq[c] += v * v
        scale = 1.0 / len(self.parts)
        mean = [s[c] * scale for c in range(2)]
        std = [math.sqrt(max(sq[c] * scale - mean[c] * mean[c], 0.0)) for c in range(2)]
        return int(mean[0] - 1.5 * std[0]), int(mean[1] - 1.5 * std[1]), int(3 * std[0]), int(3 * std[1])

    def boundingBox3D(self, im_shape, depth: np.ndarray) -> tuple:
        """Candidate.hpp:140-216 on the host, in numpy: (x, y, z, height, width, depth) (Rect3d member order, Rect3.hpp:53-64).
        `im_shape` = (rows, cols) of the colour frame, `depth` a 2-D uint8 / uint16 / float32 / float64 image of any size.
        The yardstick of pbd_boxes3d (include/pbd.h states the contract); it restates cv::resize INTER_LINEAR (float), cv::filter2D
        (float, BORDER_REFLECT_101, zero taps skipped) and getGaussianKernel.  Where the reference fails an OpenCV assertion
        (every box of zero area) the result is the NaN box, as on the device."""
        st = self.boundingBox3D_steps(im_shape, depth)
        if st is None:
            return (math.nan, math.nan, math.nan, 0.0, 0.0, 0.0)
        p = st["p"]
        bx, by, bw, bh = self.boundingBox()
        z0, z1 = float(p[st["dmin"]]), float(p[st["dmax"]])
        return float(bx), float(by), z0, float(bh), float(bw), z1 - z0

    def boundingBox3D_steps(self, im_shape, depth: np.ndarray) -> Optional[dict]:
        """boundingBox3D's intermediate results: S (the valid samples, ascending), p (the 400 resampled points), d (the filtered
        points) and the rows dmin, dmax at which the walk from the median ends; None for the NaN box"""
        S = self._samples3d(im_shape, depth)
        if S is None:
            return None
        p = _resize_linear_400(S)
        d = _dog_filter_400(p)
        dmin, dmax = _walk_400(d)
        return {"S": S, "p": p, "d": d, "dmin": dmin, "dmax": dmax}

    def _samples3d(self, im_shape, depth: np.ndarray) -> Optional[np.ndarray]:
        """the valid samples (neither 0 nor NaN as float32) of the part boxes and boundingBoxNorm(), sorted; None where the
        reference returns the NaN box (the first non-empty box holds no valid sample) or every box is empty"""
        rows, cols = int(im_shape[0]), int(im_shape[1])
        drows, dcols = depth.shape[:2]
        sx, sy = dcols / float(cols), drows / float(rows)
        boxes = [_rect_and(tuple(int(v) for v in r), (0, 0, cols, rows)) for r in self.parts]
        boxes.append(_rect_and(self.boundingBoxNorm(), (0, 0, cols, rows)))
        chunks, m = [], 0
        for x, y, w, h in boxes:
            x, y, w, h = _rect_and((int(x * sx), int(y * sy), int(w * sx), int(h * sy)), (0, 0, dcols, drows))
            if w <= 0 or h <= 0:
                continue                                      # part.empty()
            v = depth[y:y + h, x:x + w].astype(np.float32).ravel()    # Mat_<float> assignment: 64F rounds to nearest
            v = v[(v != 0) & ~np.isnan(v)]
            chunks.append(v)
            m += v.size
            if m == 0:
                return None                                   # the first non-empty box held no valid sample
        if m == 0:
            return None
        return np.sort(np.concatenate(chunks))

    @staticmethod
    def mask(im_shape, candidates: Sequence["Candidate"]) -> np.ndarray:
        """Candidate.hpp:320-331 on the host, in numpy: the CV_8U label image of `im_shape` = (rows, cols) in which label n+1 marks
        the pixels of candidate n's boundingBox() that no earlier candidate claimed (255 from n = 254 on).  The yardstick of
        pbd_candidate_mask (publish.candidate_mask)."""
        from . import publish
        return publish.candidate_mask(im_shape, [c.boundingBox() for c in candidates])

    @staticmethod
    def nonMaximaSuppression(im_shape, candidates: List["Candidate"], overlap: float = 0.0) -> None:
        """Candidate.hpp:277-304: greedy paint-the-canvas suppression on the bounding boxes, in the given
        order (callers sort by score first: cells/detect.cpp:237-238, ros/Node.cpp:192-196).  In place."""
        rows, cols = int(im_shape[0]), int(im_shape[1])
        scratch = np.zeros((rows, cols), np.uint8)
        keep = 0
        for cand in list(candidates):
            x, y, w, h = cand.boundingBox()
            x1, y1 = max(x, 0), max(y, 0)                         # box & bounds (cv::Rect operator&)
            x2, y2 = min(x + w, cols), min(y + h, rows)
            if x2 - x1 <= 0 or y2 - y1 <= 0:
                x1 = y1 = x2 = y2 = 0
            area = (x2 - x1) * (y2 - y1)
            boxsum = float(scratch[y1:y2, x1:x2].sum())
            ratio = boxsum / area if area else float("nan")       # NaN > overlap is false: an empty box is kept
            if ratio > overlap:
                continue
            scratch[y1:y2, x1:x2] = 1
            candidates[keep] = cand
            keep += 1
        del candidates[keep:]


def _rect_and(a, b):
    """cv::Rect operator& of (x, y, w, h) tuples: an empty intersection is (0, 0, 0, 0)"""
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    w, h = min(a[0] + a[2], b[0] + b[2]) - x1, min(a[1] + a[3], b[1] + b[3]) - y1
    return (x1, y1, w, h) if w > 0 and h > 0 else (0, 0, 0, 0)


def _dog_taps() -> np.ndarray:
    """filter2D(getGaussianKernel(35, 4, CV_32F), [-1 0 1]^T) (include/Candidate.hpp:190-193), float32[35]"""
    g = np.zeros(35, np.float32)
    total = 0.0
    for i in range(35):
        x = i - 17.0
        g[i] = np.float32(math.exp(-0.5 / 16.0 * x * x))
        total += float(g[i])
    total = 1.0 / total
    for i in range(35):
        g[i] = np.float32(float(g[i]) * total)
    dog = np.zeros(35, np.float32)
    for i in range(35):
        a, b = (1 if i == 0 else i - 1), (33 if i == 34 else i + 1)
        dog[i] = (np.float32(0) + np.float32(-1) * g[a]) + np.float32(1) * g[b]
    return dog


def _dog_filter_400(p: np.ndarray) -> np.ndarray:
    """cv::filter2D(p, -1, dog) of the 400 points: float32, BORDER_REFLECT_101, zero taps skipped, taps added in order"""
    d = np.zeros(400, np.float32)
    idx = np.arange(400)
    with np.errstate(invalid="ignore", over="ignore"):
        for t, k in enumerate(_dog_taps()):
            if k == 0:
                continue
            j = np.abs(idx + t - 17)
            j = np.where(j >= 400, 2 * 399 - j, j)
            d = d + k * p[j]
    return d


def _walk_400(d: np.ndarray):
    """Candidate.hpp:197-205: from row 200 out, the last rows (dmin, dmax) before |d| > 0.035"""
    mid = 200
    dmax = dmin = mid
    for m_ in range(mid, 400):
        if float(abs(d[m_])) > 0.035:
            break
        dmax = m_
    for m_ in range(mid, -1, -1):
        if float(abs(d[m_])) > 0.035:
            break
        dmin = m_
    return dmin, dmax


def _resize_linear_400(S: np.ndarray) -> np.ndarray:
    """cv::resize(S, Size(1, 400), INTER_LINEAR) of a sorted float32 column: p = S[r0] * (1 - fy) + S[r1] * fy in float32"""
    M = S.size
    if M == 400:
        return S.copy()
    scale = 1.0 / (400.0 / M)
    fy = ((np.arange(400) + 0.5) * scale - 0.5).astype(np.float32)
    sy = np.floor(fy)
    fy = (fy - sy).astype(np.float32)
    sy = sy.astype(np.int64)
    r0, r1 = np.clip(sy, 0, M - 1), np.clip(sy + 1, 0, M - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return S[r0] * (np.float32(1) - fy) + S[r1] * fy


def is_device_frame(f) -> bool:
    """a torch tensor on a GPU (anything else is taken as a host array)"""
    return hasattr(f, "data_ptr") and hasattr(f, "is_cuda") and bool(f.is_cuda)


def frame_dtype(f) -> np.dtype:
    """the numpy dtype of a host array or a torch tensor"""
    return np.dtype(str(f.dtype).replace("torch.", ""))


def device_frames(tensors):
    """(descriptors (pointer, rows, cols, pitch), channels, depth code) of torch tensors on the device, rows x cols [x cn] with
    contiguous pixels: a view of a larger image is described in place, nothing is copied"""
    if not tensors:
        raise PbdError(-1, "no frames")
    dt, cn = frame_dtype(tensors[0]), 1 if tensors[0].ndim == 2 else int(tensors[0].shape[2])
    if dt not in _lib.DEPTH_CODE:
        raise PbdError(-1, "frames are uint8, uint16, float32 or float64")
    descs = []
    for t in tensors:
        if not is_device_frame(t) or t.ndim not in (2, 3) or frame_dtype(t) != dt or (1 if t.ndim == 2 else int(t.shape[2])) != cn:
            raise PbdError(-1, "one call takes device tensors of one dtype and one channel count")
        if (t.shape[1] > 1 and t.stride(1) != cn) or (t.ndim == 3 and cn > 1 and t.stride(2) != 1):
            raise PbdError(-1, "a device frame must have contiguous pixels")
        descs.append((t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)) * t.element_size()))
    return descs, cn, _lib.DEPTH_CODE[dt]


class Handle:
    """Owns a pbd_handle (one handle = one host thread = one GPU)."""

    def __init__(self, model, device: int = 0, conv_mode: int = _lib.CONV_EXACT, max_batch: int = 1,
                 max_candidates: int = 1 << 18, stream: Optional[int] = None, real_type: int = _lib.REAL_F32):
        self.lib = _lib.load()
        self.flat: FlatModel = model if isinstance(model, FlatModel) else model.flatten()
        self._cm = _lib.c_model(self.flat)
        cfg = _lib.CConfig(device, real_type, conv_mode, max_batch, max_candidates, stream)
        h = C.c_void_p()
        rc = self.lib.pbd_create(C.byref(self._cm), C.byref(cfg), C.byref(h))
        if rc != _lib.PBD_OK:
            raise PbdError(rc, self.lib.pbd_last_error(None).decode())
        self.h = h
        self.dtype = np.float32 if real_type == _lib.REAL_F32 else np.float64   # reference template parameter T
        self.max_batch = max_batch
        self.max_candidates = max_candidates
        self.stride = self.lib.pbd_candidate_stride(self.h)
        self.max_parts = (self.stride - 8) // 4         # part boxes a record holds (pbd_candidate_stride)
        self.nms_overlap = None                          # the overlap of set_nms (None: off)
        self.level_shapes = None                         # (rows, cols) of every level of the last detect / min call (max-marginals)
        self._model_stale = False                        # set_model_vector* / set_thresh: `flat` is behind the handle
        self._thresh = None
        self._buf = None                                 # the record buffer of the pipelined and device-batch calls, reused

    def close(self):
        if getattr(self, "h", None):
            self.lib.pbd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, allow=()):
        if rc != _lib.PBD_OK and rc not in allow:
            raise PbdError(rc, self.lib.pbd_last_error(self.h).decode())
        return rc

    def stream_ptr(self) -> int:
        """pbd_stream: the hipStream_t the handle's kernels run on (wrap it with torch.cuda.ExternalStream to order torch work behind it)"""
        return int(self.lib.pbd_stream(self.h) or 0)

    def set_level_shard(self, rank: int, world: int) -> None:
        """pbd_set_level_shard: this handle computes only its share of the pyramid levels of each frame"""
        self.check(self.lib.pbd_set_level_shard(self.h, rank, world))

    def set_padding(self, padx: int, pady: int) -> None:
        """pbd_set_padding: every plan the handle builds afterwards pads its feature levels by (padx, pady) cells holding 0 on
        channels 0 .. 30 and 1 on channel 31 (the padded pyramid of featpyramid.m; padding.py states the rule); (0, 0): off.
        Roots and cells are then plane coordinates: the image cell is root_x - padx"""
        self.check(self.lib.pbd_set_padding(self.h, int(padx), int(pady)))

    def set_fine_octave(self, on: bool) -> None:
        """pbd_set_fine_octave: every image plan the handle builds afterwards has nfine = min(interval, nlevels) more levels in
        front -- reference level i's image at bin size sbin / 2, scale halved (fineoctave.py states the rule); levels index the
        longer list"""
        self.check(self.lib.pbd_set_fine_octave(self.h, 1 if on else 0))

    def set_nms(self, overlap: Optional[float]) -> None:
        """pbd_set_nms: every detect* call of this handle returns, per frame, Candidate.sort + Candidate.nonMaximaSuppression(
        (rows, cols), candidates, overlap) of what it found, computed on the device (cells/detect.cpp:237-238,
        ros/Node.cpp:192-196); None: off (the default).  `overlap` crosses the ABI as a float."""
        self.check(self.lib.pbd_set_nms(self.h, int(overlap is not None), float(overlap or 0.0)))
        self.nms_overlap = overlap

    def set_walk(self, mode: int) -> None:
        """pbd_set_walk: _lib.WALK_REFERENCE (the default: the reference's composed back-pointers) or _lib.WALK_ARGMAX (the
        placement the score was taken at) for every walk the handle makes afterwards: part boxes, examples, latent positives"""
        self.check(self.lib.pbd_set_walk(self.h, int(mode)))

    def set_root_nms(self, sz: int) -> None:
        """pbd_set_root_nms: every detect* call of this handle keeps only the roots that are grid maxima of their (frame, level,
        component) plane of rootv among the cells above the threshold (gridnms.grid_nms_ref(rootv, sz, rootv > thresh)), before
        the walk; 0: off (the default)"""
        self.check(self.lib.pbd_set_root_nms(self.h, int(sz)))

    def grid_nms(self, planes: Sequence[np.ndarray], sz: int, masks: Optional[Sequence[Optional[np.ndarray]]] = None) -> List[np.ndarray]:
        """pbd_grid_nms: nonMaximaSuppression(plane, sz, dst, mask) of every plane (2-D, all float32 or all float64, any sizes, empty
        ones included), one launch; masks: None, or one uint8 / bool plane per plane.  Returns the uint8 planes of 0 / 255.
        Equal to gridnms.grid_nms_ref."""
        planes, real, src, msk = _lib.pack_arrays(planes, masks, "grid_nms")
        if any(a.ndim != 2 for a in planes):
            raise PbdError(-1, "grid_nms: 2-D planes")
        _, _, rows, cols = _lib.shape_arrays([a.shape for a in planes])
        dst = np.zeros(src.size, np.uint8)
        self.check(self.lib.pbd_grid_nms(self.h, len(planes), rows, cols, real, src.ctypes.data, None if msk is None else msk.ctypes.data,
                                         int(sz), dst.ctypes.data))
        return _lib.split_arrays(dst, planes)

    def grid_nms_device(self, rows: Sequence[int], cols: Sequence[int], real_code: int, d_src_ptr: int, d_mask_ptr: Optional[int],
                        sz: int, d_dst_ptr: int) -> None:
        """pbd_grid_nms_device: the packed planes at d_src_ptr (rows[i] x cols[i] each, REAL_F32 or REAL_F64), the optional packed
        mask bytes, the packed result bytes; asynchronous on the handle's stream"""
        ir, _, r, c = _lib.shape_arrays(list(zip(rows, cols)))
        self.check(self.lib.pbd_grid_nms_device(self.h, len(ir), r, c, int(real_code), d_src_ptr or None, d_mask_ptr or None, int(sz),
                                                d_dst_ptr or None))

    def set_top_k(self, k: int) -> None:
        """pbd_set_top_k: every detect* call of this handle keeps only the k best roots of each frame among the cells the threshold
        and the other root filters leave (topk.top_k_cells_ref over the frame's rootv), before the walk; 0: off (the default)"""
        self.check(self.lib.pbd_set_top_k(self.h, int(k)))

    def set_scale_nms(self, dl: Optional[int]) -> None:
        """pbd_set_scale_nms: every detect* call of this handle keeps only the roots no better root beats whose rectangle's centre
        lies in its own, or the other way round, within dl pyramid levels of the same frame (scalenms.keep_records over the
        records), after depth pruning and root NMS and before top-K; None: off (the default)"""
        self.check(self.lib.pbd_set_scale_nms(self.h, 0 if dl is None else 1, 0 if dl is None else int(dl)))

    def scale_nms(self, nframes: int, dl: int, records: np.ndarray, frame_offset: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """pbd_scale_nms: per frame the records (n, stride) no better neighbouring record beats, in input order; the records are
        grouped by ascending frame (equal to scalenms.filter_records)"""
        return self._list_call(self.lib.pbd_scale_nms, (int(nframes), int(dl)), records, frame_offset, capacity)

    def scale_nms_device(self, nframes: int, dl: int, d_payload_ptr: int, capacity: int, frame_offset: int, d_out_ptr: int,
                         out_capacity: int) -> None:
        """pbd_scale_nms_device: the records of a device payload, the kept records into the payload at d_out_ptr (word 0 = kept
        count, -1 when the input's word 0 is out of range); asynchronous on the handle's stream"""
        self.check(self.lib.pbd_scale_nms_device(self.h, int(nframes), int(dl), d_payload_ptr, capacity, frame_offset, d_out_ptr,
                                                 out_capacity))

    def top_k_cells(self, segments: Sequence[np.ndarray], k: int, masks: Optional[Sequence[Optional[np.ndarray]]] = None) -> List[np.ndarray]:
        """pbd_top_k_cells: the k best eligible elements of every segment (1-D after ravel, all float32 or all float64, any lengths,
        empty ones included), one launch sequence; masks: None, or one uint8 / bool array per segment.  Returns the uint8 arrays of
        0 / 255 in the segments' shapes.  Equal to topk.top_k_cells_ref."""
        segs, real, src, msk = _lib.pack_arrays(segments, masks, "top_k_cells")
        ln = np.array([a.size for a in segs], np.int64)
        dst = np.zeros(src.size, np.uint8)
        self.check(self.lib.pbd_top_k_cells(self.h, len(segs), _lib.ptr(ln, C.c_longlong), real, src.ctypes.data,
                                            None if msk is None else msk.ctypes.data, int(k), dst.ctypes.data))
        return _lib.split_arrays(dst, segs)

    def top_k_cells_device(self, lengths: Sequence[int], real_code: int, d_src_ptr: int, d_mask_ptr: Optional[int], k: int,
                           d_dst_ptr: int) -> None:
        """pbd_top_k_cells_device: the packed segments at d_src_ptr (lengths[i] elements each, REAL_F32 or REAL_F64), the optional
        packed mask bytes, the packed result bytes; asynchronous on the handle's stream"""
        ln = np.asarray(lengths, np.int64)
        self.check(self.lib.pbd_top_k_cells_device(self.h, len(ln), _lib.ptr(ln, C.c_longlong), int(real_code), d_src_ptr or None,
                                                   d_mask_ptr or None, int(k), d_dst_ptr or None))

    def top_k(self, nframes: int, k: int, records: np.ndarray, frame_offset: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """pbd_top_k: per frame the k best records (n, stride) by score, ties to the earlier record, in input order; the records are
        grouped by ascending frame (equal to topk.top_k_records_ref)"""
        return self._list_call(self.lib.pbd_top_k, (int(nframes), int(k)), records, frame_offset, capacity)

    def top_k_device(self, nframes: int, k: int, d_payload_ptr: int, capacity: int, frame_offset: int, d_out_ptr: int,
                     out_capacity: int) -> None:
        """pbd_top_k_device: the records of a device payload, the kept records into the payload at d_out_ptr (word 0 = kept count,
        -1 for an overflowed input); asynchronous"""
        self.check(self.lib.pbd_top_k_device(self.h, int(nframes), int(k), d_payload_ptr, capacity, frame_offset, d_out_ptr,
                                             out_capacity))

    def set_debug_option(self, option: int, value: int) -> None:
        """pbd_debug_set_option: force one of this handle's launch choices (tests), the default value restoring the automatic
        one.  _lib.DT_LANE_SHIFT: 0..6, 64 >> value rows per wave of the distance transform (-1); _lib.DT_COOP: 0, never
        its cooperative kernel (1); _lib.DT_COOP_G: 4 or 8 rows per wave of that kernel (0); _lib.DP_BUDGET_MB: > 0, the
        dynamic program's scratch per chunk of frames (0: 8 GB); _lib.GRID_NMS_LANES: 1 or 64 lanes per block of k_grid_nms (0: by sz);
        _lib.HOG_TWO_PASS: 1, the HOG histograms never take the fused gradient + histogram kernel (0)."""
        self.check(self.lib.pbd_debug_set_option(self.h, option, value))

    # ---- helpers -------------------------------------------------------------------------------
    def plan(self, rows: int, cols: int):
        n = C.c_int()
        arrs = [np.zeros(_lib.MAX_LEVELS, np.int32) for _ in range(4)]
        sc = np.zeros(_lib.MAX_LEVELS, np.float32)
        self.check(self.lib.pbd_pyramid_plan(self.h, rows, cols, C.byref(n), *[_lib.ptr(a, C.c_int) for a in arrs],
                                             _lib.ptr(sc, C.c_float)))
        k = n.value
        return {"nlevels": k, "img_rows": arrs[0][:k].copy(), "img_cols": arrs[1][:k].copy(),
                "feat_rows": arrs[2][:k].copy(), "feat_cols": arrs[3][:k].copy(), "scales": sc[:k].copy()}

    def unpack_candidates(self, buf: np.ndarray, n: int) -> List[Candidate]:
        out = []
        rec = buf[: n * self.stride].reshape(n, self.stride)
        for r in rec:
            npart = int(r[6])
            conf = np.zeros(npart, np.float32)
            conf[0] = r[5:6].view(np.float32)[0]
            out.append(Candidate(parts=r[8:8 + 4 * npart].reshape(npart, 4).copy(), confidence=conf,
                                 component=int(r[1]), frame=int(r[0]), level=int(r[2]), root=(int(r[3]), int(r[4]))))
        return out

    def pack_candidates(self, candidates: Sequence[Candidate]) -> np.ndarray:
        """records (n, stride) int32 of Candidate objects (the layout unpack_candidates reads)"""
        rec = np.zeros((len(candidates), self.stride), np.int32)
        for i, c in enumerate(candidates):
            parts = np.asarray(c.parts, np.int32).reshape(-1, 4)
            rec[i, :8] = (c.frame, c.component, c.level, c.root[0], c.root[1], 0, len(parts), 0)
            rec[i, 5] = np.float32(c.score()).view(np.int32)
            rec[i, 8:8 + parts.size] = parts.ravel()
        return rec

    def boxes3d(self, depths: Sequence[np.ndarray], im_shapes, records: np.ndarray, frame_offset: int = 0) -> np.ndarray:
        """pbd_boxes3d: Candidate::boundingBox3D of every record (n, stride) on the device, (n, 6) float64 in Rect3d member
        order.  depths[f]: 2-D depth image of frame f (one dtype for the call, rows of any pitch); im_shapes[f] = (rows, cols)
        of the colour frame; a record's frame index is its `frame` field - frame_offset."""
        ds, descs, code = _lib.depth_frames(depths)
        _, _, ir, ic = _lib.shape_arrays(im_shapes)
        rec = self._records(records)
        out = np.zeros((len(rec), 6), np.float64)
        self.check(self.lib.pbd_boxes3d(self.h, len(ds), descs, code, ir, ic, _lib.opt_ptr(rec), len(rec), frame_offset, _lib.opt_ptr(out)))
        return out

    def boxes3d_device(self, descs, depth_code: int, im_shapes, d_payload_ptr: int, capacity: int, frame_offset: int,
                       d_out_ptr: int) -> None:
        """pbd_boxes3d_device: the records of a device payload (as detect_batch_device_out leaves it), depth frames
        (device pointer, rows, cols, pitch), boxes into double[6 * capacity] at d_out_ptr; asynchronous on the handle's stream"""
        _, _, ir, ic = _lib.shape_arrays(im_shapes)
        self.check(self.lib.pbd_boxes3d_device(self.h, len(descs), _lib.frame_array(descs), depth_code, ir, ic, d_payload_ptr, capacity,
                                               frame_offset, d_out_ptr))

    def _records(self, records) -> np.ndarray:
        return np.ascontiguousarray(records, np.int32).reshape(-1, self.stride)

    def _list_call(self, fn, args, records, frame_offset: int, capacity: Optional[int]) -> np.ndarray:
        """a host list-in / list-out entry point, fn(h, *args, records, n, frame_offset, out, capacity, &kept): the kept records.
        capacity None: room for every record.  More kept than the capacity is the library's PBD_ERR_CAPACITY."""
        rec = self._records(records)
        cap = len(rec) if capacity is None else capacity
        out = np.zeros((max(cap, 1), self.stride), np.int32)
        n = C.c_int()
        self.check(fn(self.h, *args, _lib.opt_ptr(rec), len(rec), frame_offset, out.ctypes.data, cap, C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def _host_list(self, fn, args, capacity: Optional[int], raw: bool = False, cached: bool = False):
        """a detect-family entry point that lists its records on the host, fn(h, *args, buf, capacity, &n): the list as Candidates,
        or as (buf, n) for raw.  capacity None: max_candidates.  cached: into the handle's own buffer, grown on demand and reused
        (nothing is allocated per call; a raw result is valid until the next cached call), else into a new one."""
        cap = self.max_candidates if capacity is None else capacity
        buf = getattr(self, "_buf", None) if cached else None
        if buf is None or buf.size < cap * self.stride:
            buf = np.zeros(max(cap, 1) * self.stride, np.int32)
            if cached:
                self._buf = buf
        n = C.c_int()
        self.check(fn(self.h, *args, buf.ctypes.data, cap, C.byref(n)))
        return (buf, n.value) if raw else self.unpack_candidates(buf, n.value)

    def synchronize(self) -> None:
        """pbd_synchronize: wait for everything enqueued on the handle's stream"""
        self.check(self.lib.pbd_synchronize(self.h))

    def binsize(self) -> int:
        return self.lib.pbd_binsize(self.h)

    def model_vector_len(self) -> int:
        return self.lib.pbd_model_vector_len(self.h)

    def model_vector(self) -> np.ndarray:
        """pbd_model_vector: w = [biasw | defw | filters] in T"""
        w = np.zeros(self.model_vector_len(), self.dtype)
        self.check(self.lib.pbd_model_vector(self.h, w.ctypes.data))
        return w

    def set_model_vector(self, w) -> None:
        """pbd_set_model_vector: the handle's parameters become w (model_vector()'s order, rounded to T), in place: afterwards
        the handle equals a new one created from Model.from_vector(w).  The resident detect result is dropped."""
        w = np.ascontiguousarray(w, self.dtype).ravel()
        n = self.model_vector_len()
        if len(w) != n:
            raise PbdError(-1, f"model vector of {len(w)} values, this handle's has {n}")
        self.check(self.lib.pbd_set_model_vector(self.h, w.ctypes.data))
        self._model_stale = True

    def set_model_vector_device(self, d_w_ptr: int, dtype) -> None:
        """pbd_set_model_vector_device: the same from model_vector_len float32 / float64 values on the handle's device (the
        caller orders their producer before stream_ptr()); nothing of the bank's size crosses to the host"""
        self.check(self.lib.pbd_set_model_vector_device(self.h, d_w_ptr, _lib.real_code(dtype)))
        self._model_stale = True

    def set_thresh(self, thresh: float) -> None:
        """pbd_set_thresh: the model's threshold for every later detect call"""
        self.check(self.lib.pbd_set_thresh(self.h, float(thresh)))
        self._thresh = float(np.float32(thresh))
        self._model_stale = True

    def current_model(self):
        """the Model the handle holds now: the one it was created from, with the parameters of the last update (fetched from
        the handle when asked, not at the update) and the last set_thresh"""
        if self._model_stale:
            m = self.flat.model.from_vector(self.model_vector())
            if self._thresh is not None:
                m.thresh = self._thresh
            self.flat = m.flatten()
            self._model_stale = False
        return self.flat.model

    def example_stride(self):
        """pbd_example_stride: (int32 words of a header, values of T of an example)"""
        a, b = C.c_int(), C.c_int()
        self.check(self.lib.pbd_example_stride(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def examples(self, records: np.ndarray, frame_offset: int = 0):
        """pbd_examples: (hdr (n, hdr_words) int32, values (n, values) T) of records (n, stride) of the last detect call"""
        rec = self._records(records)
        hw, vw = self.example_stride()
        hdr = np.zeros((len(rec), hw), np.int32)
        vals = np.zeros((len(rec), vw), self.dtype)
        self.check(self.lib.pbd_examples(self.h, _lib.opt_ptr(rec), len(rec), frame_offset, _lib.opt_ptr(hdr), _lib.opt_ptr(vals)))
        return hdr, vals

    def part_scores(self, records: np.ndarray, frame_offset: int = 0, fill=0):
        """pbd_part_scores: (status (n,) int32, place (n, max_parts, 3) int32 x, y, m, scores (n, max_parts, 4) T appearance,
        message, bias, total) of records (n, stride) of the last detect call, at the walk's placement.  Entries past a record's
        parts keep `fill`."""
        rec, ptr = self._records(records), _lib.opt_ptr
        status = np.full(len(rec), fill, np.int32)
        place = np.full((len(rec), self.max_parts, 3), fill, np.int32)
        scores = np.full((len(rec), self.max_parts, 4), fill, self.dtype)
        self.check(self.lib.pbd_part_scores(self.h, ptr(rec), len(rec), frame_offset, ptr(status), ptr(place), ptr(scores)))
        return status, place, scores

    def score_placements(self, records: np.ndarray, place: np.ndarray, frame_offset: int = 0, fill=0):
        """pbd_score_placements: (status (n,) int32, scores (n, max_parts, 4) T) of the placements place (n, max_parts, 3) x, y, m
        (place[i][0] the root) in the frame, level and component of records (n, stride); a placement outside the map or the
        part's mixtures has status -1 and keeps `fill`"""
        rec, ptr = self._records(records), _lib.opt_ptr
        place = np.ascontiguousarray(place, np.int32)
        if place.shape != (len(rec), self.max_parts, 3):
            raise PbdError(-1, f"placements of shape {place.shape}, expected {(len(rec), self.max_parts, 3)}")
        status = np.full(len(rec), fill, np.int32)
        scores = np.full((len(rec), self.max_parts, 4), fill, self.dtype)
        self.check(self.lib.pbd_score_placements(self.h, ptr(rec), len(rec), frame_offset, ptr(place), ptr(status), ptr(scores)))
        return status, scores

    def part_scores_device(self, d_payload_ptr: int, capacity: int, frame_offset: int, d_status_ptr: int, d_place_ptr,
                           d_scores_ptr: int) -> None:
        """pbd_part_scores_device: status int32[capacity], place int32[capacity * max_parts * 3] (or None) and scores
        T[capacity * max_parts * 4] of a device payload's records; asynchronous on the handle's stream"""
        self.check(self.lib.pbd_part_scores_device(self.h, d_payload_ptr, capacity, frame_offset, d_status_ptr, d_place_ptr,
                                                   d_scores_ptr))

    def score_placements_device(self, d_payload_ptr: int, capacity: int, frame_offset: int, d_place_ptr: int, d_status_ptr: int,
                                d_scores_ptr: int) -> None:
        """pbd_score_placements_device: score_placements on device arrays; asynchronous on the handle's stream"""
        self.check(self.lib.pbd_score_placements_device(self.h, d_payload_ptr, capacity, frame_offset, d_place_ptr, d_status_ptr,
                                                        d_scores_ptr))

    def max_marginals(self, frame: int = 0) -> None:
        """pbd_max_marginals: the max-marginal planes of one frame of the resident dynamic-program result, kept on the device until
        the next detect call, min(), model update or max_marginals; asynchronous on the handle's stream"""
        self.check(self.lib.pbd_max_marginals(self.h, int(frame)))

    def get_marginals(self, level: int, what: int, rows: int, cols: int) -> np.ndarray:
        """pbd_get_marginals: one level's block (NJ, rows, cols): T for _lib.MM_VALUES / MM_DOWN, int32 for MM_PARENT_X / _Y / _K"""
        nj = int(self.flat.mix_offset[-1])
        dst = np.empty((nj, rows, cols), self.dtype if what in (_lib.MM_VALUES, _lib.MM_DOWN) else np.int32)
        self.check(self.lib.pbd_get_marginals(self.h, int(level), int(what), dst.ctypes.data, dst.nbytes))
        return dst

    def marginals_device(self, level: int) -> int:
        """pbd_marginals_device: the device address of the level's mm block T[NJ][rows][cols]"""
        p = C.c_void_p()
        self.check(self.lib.pbd_marginals_device(self.h, int(level), C.byref(p)))
        return int(p.value or 0)

    def marginal_poses(self, seeds, scales=None, frame_offset: int = 0, fill=0):
        """pbd_marginal_poses: (status (n,) int32, records (n, stride) int32, place (n, max_parts, 3) int32 x, y, type) of the seeds
        (n, 6) int32 {level, component, part, type or -1, x, y}; scales None: the resident plan's own (after a detect call).  A bad
        seed has status -1 and keeps `fill`, as the entries past a pose's parts do."""
        sd = np.ascontiguousarray(seeds, np.int32).reshape(-1, 6)
        n = len(sd)
        status = np.full(n, fill, np.int32)
        rec = np.full((n, self.stride), fill, np.int32)
        place = np.full((n, self.max_parts, 3), fill, np.int32)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        ptr = _lib.opt_ptr
        self.check(self.lib.pbd_marginal_poses(self.h, n, ptr(sd), None if sc is None else _lib.ptr(sc, C.c_float), frame_offset,
                                               ptr(rec), ptr(place), ptr(status)))
        return status, rec, place

    def marginal_poses_device(self, n: int, d_seeds_ptr: int, scales, frame_offset: int, d_cand_ptr: int, d_place_ptr,
                              d_status_ptr: int) -> None:
        """pbd_marginal_poses_device: marginal_poses on device arrays (d_place_ptr may be None); asynchronous on the handle's
        stream"""
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        self.check(self.lib.pbd_marginal_poses_device(self.h, int(n), d_seeds_ptr or None, None if sc is None else _lib.ptr(sc, C.c_float),
                                                      frame_offset, d_cand_ptr or None, d_place_ptr or None, d_status_ptr or None))

    def detect_latent(self, frames, part_boxes, overlap: float, mixtures=None):
        """pbd_detect_latent: (records (nframes, stride) int32, found (nframes,) int32) -- per frame the best root whose parts
        overlap part_boxes[f][p] = (x1, y1, x2, y2) inclusive by more than `overlap`; mixtures[f][p]: fixed mixture or -1"""
        fr, descs, cn, code = _lib.image_frames(frames)
        boxes = np.ascontiguousarray(part_boxes, np.int32).reshape(len(fr), -1, 4)
        mix = None if mixtures is None else np.ascontiguousarray(mixtures, np.int32).reshape(len(fr), boxes.shape[1])
        if mix is not None and mix.shape != boxes.shape[:2]:
            raise PbdError(-1, "one mixture per part box")
        rec = np.zeros((len(fr), self.stride), np.int32)
        found = np.zeros(len(fr), np.int32)
        self.check(self.lib.pbd_detect_latent(self.h, len(fr), descs, cn, code, boxes.ctypes.data, None if mix is None else mix.ctypes.data,
                                              float(overlap), rec.ctypes.data, found.ctypes.data))
        return rec, found

    def detect_latent_device(self, descs, cn: int, depth_code: int, part_boxes, overlap: float, mixtures=None):
        """pbd_detect_latent_device: detect_latent on frames already on the device as (pointer, rows, cols, pitch), regions of
        larger images included; the boxes, the mixtures and the result are host arrays and the call is synchronous"""
        boxes = np.ascontiguousarray(part_boxes, np.int32).reshape(len(descs), -1, 4)
        mix = None if mixtures is None else np.ascontiguousarray(mixtures, np.int32).reshape(len(descs), boxes.shape[1])
        rec = np.zeros((len(descs), self.stride), np.int32)
        found = np.zeros(len(descs), np.int32)
        self.check(self.lib.pbd_detect_latent_device(self.h, len(descs), _lib.frame_array(descs), cn, depth_code, boxes.ctypes.data,
                                                     None if mix is None else mix.ctypes.data, float(overlap), rec.ctypes.data,
                                                     found.ctypes.data))
        return rec, found

    def augment_plan(self, rows: int, cols: int, degrees: float):
        """pbd_augment_plan: (out_rows, out_cols, (c, s)) of a rows x cols frame turned by `degrees`"""
        r, c, coef = C.c_int(), C.c_int(), (C.c_double * 2)()
        rc = self.lib.pbd_augment_plan(int(rows), int(cols), float(degrees), C.byref(r), C.byref(c), coef)
        if rc != _lib.PBD_OK:
            raise PbdError(rc, self.lib.pbd_last_error(None).decode())
        return r.value, c.value, (coef[0], coef[1])

    def augment_frames(self, frames, jobs, outs=None):
        """pbd_augment_frames: the copies rotate(mirror(frames[f])) of jobs (n, 3) = (frame, mirror, degrees) as host arrays;
        frames are arrays of one dtype and channel count, any sizes.  outs: destinations to write into (views with padded rows
        allowed), else new arrays."""
        fr, descs, cn, code = _lib.image_frames(frames)
        jobs = [(int(f), bool(m), float(d)) for f, m, d in jobs]
        if outs is None:
            outs = []
            for f, _, d in jobs:
                if not 0 <= f < len(fr):
                    raise PbdError(-1, f"frame {f} outside 0..{len(fr) - 1}")
                r, c, _ = self.augment_plan(fr[f].shape[0], fr[f].shape[1], d)
                outs.append(np.zeros((r, c, fr[f].shape[2]), fr[f].dtype))
        odesc = _lib.frame_array([(o.ctypes.data, o.shape[0], o.shape[1], o.strides[0]) for o in outs])
        self.check(self.lib.pbd_augment_frames(self.h, len(fr), descs, cn, code, len(jobs), _lib.augment_array(jobs), odesc))
        return outs

    def augment_frames_device(self, descs, cn: int, depth_code: int, jobs, out_descs) -> None:
        """pbd_augment_frames_device: frames and destinations as (device pointer, rows, cols, pitch); asynchronous on the
        handle's stream"""
        self.check(self.lib.pbd_augment_frames_device(self.h, len(descs), _lib.frame_array(descs), cn, depth_code, len(jobs),
                                                      _lib.augment_array(jobs), _lib.frame_array(out_descs)))

    def examples_device(self, d_payload_ptr: int, capacity: int, frame_offset: int, d_hdr_ptr: int, d_values_ptr: int) -> None:
        """pbd_examples_device: the examples of a device payload's records into int32[capacity * hdr_words] and
        T[capacity * values] on the device; asynchronous on the handle's stream"""
        self.check(self.lib.pbd_examples_device(self.h, d_payload_ptr, capacity, frame_offset, d_hdr_ptr, d_values_ptr))

    def warp_positives(self, frames, boxes, filter: int = 0, bias: int = 0, skip_small: bool = True):
        """pbd_warp_positives: (hdr (n, hdr_words) int32, values (n, values) T, kept (n,) int32) of boxes (n, 5) = frame, x1, y1,
        x2, y2 (0-based, inclusive) in `frames` (arrays of one dtype and channel count, any sizes): every box padded by one cell,
        cropped with edge replication, resized to (k + 2) * sbin pixels, its HOG as the example [bias = 1 | filter block];
        a box skipped as too small has hdr[2] = -1.  Values past nvalues and the rows of skipped boxes stay 0.  The resident
        detect result is dropped."""
        fr, descs, cn, code = _lib.image_frames(frames)
        bx = np.ascontiguousarray(boxes, np.int32).reshape(-1, 5)
        hw, vw = self.example_stride()
        hdr = np.zeros((len(bx), hw), np.int32)
        vals = np.zeros((len(bx), vw), self.dtype)
        kept = np.zeros(len(bx), np.int32)
        self.check(self.lib.pbd_warp_positives(self.h, len(fr), descs, cn, code, len(bx), _lib.opt_ptr(bx), filter, bias,
                                               1 if skip_small else 0, _lib.opt_ptr(hdr), _lib.opt_ptr(vals), _lib.opt_ptr(kept)))
        return hdr, vals, kept

    def warp_positives_device(self, descs, cn: int, depth_code: int, boxes, filter: int, bias: int, skip_small: bool, id_offset: int,
                              d_payload_ptr: int, capacity: int, d_hdr_ptr: int, d_values_ptr: int) -> None:
        """pbd_warp_positives_device: frames (device pointer, rows, cols, pitch), boxes (n, 5) on the host; the examples into
        int32[capacity * hdr_words] / T[capacity * values] and the payload int32[1 + capacity * stride] (word 0 = n, record i =
        {id_offset + i, 0 ...}) on the device, ready for QP.add_device; asynchronous on the handle's stream"""
        bx = np.ascontiguousarray(boxes, np.int32).reshape(-1, 5)
        self.check(self.lib.pbd_warp_positives_device(self.h, len(descs), _lib.frame_array(descs), cn, depth_code, len(bx),
                                                      _lib.opt_ptr(bx), filter, bias, 1 if skip_small else 0, id_offset, d_payload_ptr,
                                                      capacity, d_hdr_ptr, d_values_ptr))

    def depth_consistency(self, depths: Sequence[np.ndarray], records: np.ndarray, zfactor: float = 0.03, frame_offset: int = 0,
                          capacity: Optional[int] = None) -> np.ndarray:
        """pbd_depth_consistency: the records (n, stride) that SearchSpacePruning::filterCandidatesByDepth keeps, in input order,
        computed on the device.  depths[f]: the 2-D depth image of frame index f (one dtype per call, rows of any pitch)."""
        ds, descs, code = _lib.depth_frames(depths)
        return self._list_call(self.lib.pbd_depth_consistency, (len(ds), descs, code, float(zfactor)), records, frame_offset, capacity)

    def depth_consistency_device(self, descs, depth_code: int, zfactor: float, d_payload_ptr: int, capacity: int, frame_offset: int,
                                 d_out_ptr: int, out_capacity: int) -> None:
        """pbd_depth_consistency_device: the records of a device payload, depth frames (device pointer, rows, cols, pitch), the kept
        records into the payload at d_out_ptr (word 0 = kept count, -1 for an overflowed input); asynchronous"""
        self.check(self.lib.pbd_depth_consistency_device(self.h, len(descs), _lib.frame_array(descs), depth_code, float(zfactor),
                                                         d_payload_ptr, capacity, frame_offset, d_out_ptr, out_capacity))

    _depth_frames = staticmethod(_lib.depth_frames)     # the names the raw-call tests build their arguments with
    _prune_cfg = staticmethod(_lib.prune_cfg)

    def set_depth_prune(self, fx: Optional[float], width: float = 0.0, tol: float = 0.3) -> None:
        """pbd_set_depth_prune: with depth images bound (bind_depth), every detect* call of this handle lists only the roots whose
        rectangle is depthprune.plausible(rect, depth, fx, width, tol); fx None: off (the default)"""
        self.check(self.lib.pbd_set_depth_prune(self.h, None if fx is None else _lib.prune_cfg(fx, width, tol)))

    def bind_depth(self, depths: Optional[Sequence[np.ndarray]]) -> None:
        """pbd_bind_depth: the depth images (one per frame, the frame's rows x cols) of the NEXT detect* call or argmin_device_out,
        copied now; None or []: unbind"""
        if not depths:
            self.check(self.lib.pbd_bind_depth(self.h, 0, None, 0))
            return
        ds, descs, code = _lib.depth_frames(depths)
        self.check(self.lib.pbd_bind_depth(self.h, len(ds), descs, code))

    def bind_depth_device(self, descs, depth_code: int) -> None:
        """pbd_bind_depth_device: the same for depth frames (device pointer, rows, cols, pitch) read in place by the next call"""
        self.check(self.lib.pbd_bind_depth_device(self.h, len(descs), _lib.frame_array(descs) if len(descs) else None, depth_code))

    def depth_prune(self, depths: Sequence[np.ndarray], records: np.ndarray, fx: float, width: float, tol: float,
                    frame_offset: int = 0, capacity: Optional[int] = None) -> np.ndarray:
        """pbd_depth_prune: the records (n, stride) whose root rectangle is plausible in their frame's depth image, in input order,
        decided on the device (equal to depthprune.filter_records)"""
        ds, descs, code = _lib.depth_frames(depths)
        return self._list_call(self.lib.pbd_depth_prune, (_lib.prune_cfg(fx, width, tol), len(ds), descs, code), records, frame_offset,
                               capacity)

    def depth_prune_device(self, descs, depth_code: int, fx: float, width: float, tol: float, d_payload_ptr: int, capacity: int,
                           frame_offset: int, d_out_ptr: int, out_capacity: int) -> None:
        """pbd_depth_prune_device: the records of a device payload, depth frames (device pointer, rows, cols, pitch), the kept
        records into the payload at d_out_ptr (word 0 = kept count, -1 for an overflowed input); asynchronous"""
        self.check(self.lib.pbd_depth_prune_device(self.h, _lib.prune_cfg(fx, width, tol), len(descs), _lib.frame_array(descs),
                                                   depth_code, d_payload_ptr, capacity, frame_offset, d_out_ptr, out_capacity))

    def suppress(self, im_shapes, overlap: float, records: np.ndarray, frame_offset: int = 0,
                 capacity: Optional[int] = None) -> np.ndarray:
        """pbd_suppress: per frame Candidate.sort + Candidate.nonMaximaSuppression((rows, cols), ., overlap) of records grouped by
        ascending frame (the pbd_set_nms stage on a caller's list); im_shapes[f] = (rows, cols) of frame index f"""
        ir, _, pr, pc = _lib.shape_arrays(im_shapes)
        return self._list_call(self.lib.pbd_suppress, (len(ir), pr, pc, float(overlap)), records, frame_offset, capacity)

    def suppress_device(self, im_shapes, overlap: float, d_payload_ptr: int, capacity: int, frame_offset: int, d_out_ptr: int,
                        out_capacity: int) -> None:
        """pbd_suppress_device: suppress on a device payload's records, the kept records into the payload at d_out_ptr (word 0 =
        kept count, -1 for an overflowed input); asynchronous"""
        ir, _, pr, pc = _lib.shape_arrays(im_shapes)
        self.check(self.lib.pbd_suppress_device(self.h, len(ir), pr, pc, float(overlap), d_payload_ptr, capacity, frame_offset, d_out_ptr,
                                                out_capacity))

    # ---- testing a model (include/pbd.h; the numpy yardstick is evaluation.py) ----------------------
    def eval_nparts(self) -> int:
        """the one part count the evaluation calls read every record with"""
        po = self.flat.part_offset
        return int(po[1] - po[0])

    def part_nms(self, nframes: int, overlap: float, records: np.ndarray, max_boxes: int = 1000, frame_offset: int = 0,
                 capacity: Optional[int] = None) -> np.ndarray:
        """pbd_part_nms: matlab/detection/nms.m per frame of records grouped by ascending frame; the kept records, frame by
        frame, in pick order"""
        return self._list_call(self.lib.pbd_part_nms, (nframes, float(overlap), max_boxes), records, frame_offset, capacity)

    def part_nms_device(self, nframes: int, overlap: float, max_boxes: int, d_payload_ptr: int, capacity: int, frame_offset: int,
                        d_out_ptr: int, out_capacity: int) -> None:
        """pbd_part_nms_device: a device payload in, the kept records into the payload at d_out_ptr (word 0 = kept count, -1 for
        a bad list); asynchronous"""
        self.check(self.lib.pbd_part_nms_device(self.h, nframes, float(overlap), max_boxes, d_payload_ptr, capacity, frame_offset,
                                                d_out_ptr, out_capacity))

    def best_overlap(self, gtboxes, overlap: float, records: np.ndarray, frame_offset: int = 0):
        """pbd_best_overlap: matlab/detection/bestoverlap.m per frame.  gtboxes (nframes, 4) float64 x1, y1, x2, y2 (a NaN row:
        no ground truth) -> records (nframes, stride), found (nframes,) int32"""
        gt = np.ascontiguousarray(gtboxes, np.float64).reshape(-1, 4)
        rec = self._records(records)
        out = np.zeros((len(gt), self.stride), np.int32)
        found = np.zeros(len(gt), np.int32)
        self.check(self.lib.pbd_best_overlap(self.h, len(gt), gt.ctypes.data, float(overlap), _lib.opt_ptr(rec), len(rec), frame_offset,
                                             out.ctypes.data, found.ctypes.data))
        return out, found

    def best_overlap_device(self, gtboxes, overlap: float, d_payload_ptr: int, capacity: int, frame_offset: int, d_out_ptr: int,
                            d_found_ptr: int) -> None:
        """pbd_best_overlap_device: a device payload in, int32[nframes][stride] at d_out_ptr and int32[nframes] at d_found_ptr;
        asynchronous"""
        gt = np.ascontiguousarray(gtboxes, np.float64).reshape(-1, 4)
        self.check(self.lib.pbd_best_overlap_device(self.h, len(gt), gt.ctypes.data, float(overlap), d_payload_ptr, capacity,
                                                    frame_offset, d_out_ptr, d_found_ptr))

    def _pck_args(self, nframes: int, gt_points, scale):
        gt = np.ascontiguousarray(gt_points, np.float64)
        sc = np.ascontiguousarray(scale, np.float64)
        if gt.size != nframes * self.eval_nparts() * 2 or sc.size != nframes:
            raise PbdError(-1, f"gt_points is (nframes, {self.eval_nparts()}, 2) and scale (nframes,)")
        return gt, sc

    def eval_pck(self, records: np.ndarray, found, gt_points, scale, thresh: float = 0.5, want_dist: bool = True):
        """pbd_eval_pck: matlab/evaluation/eval_pck.m on one record per frame (best_overlap's output) -> pck (nparts,), dist
        (nparts, nframes) or None"""
        rec = self._records(records)
        fnd = np.ascontiguousarray(found, np.int32)
        gt, sc = self._pck_args(len(rec), gt_points, scale)
        npart = self.eval_nparts()
        pck = np.zeros(npart)
        dist = np.zeros((npart, len(rec))) if want_dist else None
        self.check(self.lib.pbd_eval_pck(self.h, len(rec), rec.ctypes.data, fnd.ctypes.data, gt.ctypes.data, sc.ctypes.data,
                                         float(thresh), pck.ctypes.data, dist.ctypes.data if want_dist else None))
        return pck, dist

    def eval_pck_device(self, nframes: int, d_rec_ptr: int, d_found_ptr: int, gt_points, scale, thresh: float, d_pck_ptr: int,
                        d_dist_ptr: Optional[int]) -> None:
        """pbd_eval_pck_device: best_overlap_device's outputs in, double[nparts] at d_pck_ptr and, unless None,
        double[nparts][nframes] at d_dist_ptr; asynchronous"""
        gt, sc = self._pck_args(nframes, gt_points, scale)
        self.check(self.lib.pbd_eval_pck_device(self.h, nframes, d_rec_ptr, d_found_ptr, gt.ctypes.data, sc.ctypes.data, float(thresh),
                                                d_pck_ptr, d_dist_ptr))

    def _apk_args(self, gt_offset, gt_points, gt_scale):
        off = np.ascontiguousarray(gt_offset, np.int32)
        gt = np.ascontiguousarray(gt_points, np.float64)
        sc = np.ascontiguousarray(gt_scale, np.float64)
        if len(off) < 2 or gt.size != int(off[-1]) * self.eval_nparts() * 2 or sc.size != int(off[-1]):
            raise PbdError(-1, f"gt_offset is (nframes + 1,), gt_points (G, {self.eval_nparts()}, 2) and gt_scale (G,), G = gt_offset[-1]")
        return off, gt, sc

    def eval_apk(self, records: np.ndarray, gt_offset, gt_points, gt_scale, thresh: float = 0.5, frame_offset: int = 0,
                 want_curves: bool = True):
        """pbd_eval_apk: matlab/evaluation/eval_apk.m + VOCap.m for every part -> apk (nparts,), prec, rec (nparts, n) or None"""
        rec = self._records(records)
        off, gt, sc = self._apk_args(gt_offset, gt_points, gt_scale)
        npart = self.eval_nparts()
        apk = np.zeros(npart)
        prec = np.zeros((npart, len(rec))) if want_curves else None
        rcl = np.zeros((npart, len(rec))) if want_curves else None
        self.check(self.lib.pbd_eval_apk(self.h, len(off) - 1, off.ctypes.data, gt.ctypes.data, sc.ctypes.data, float(thresh),
                                         _lib.opt_ptr(rec), len(rec), frame_offset, apk.ctypes.data,
                                         prec.ctypes.data if want_curves else None, rcl.ctypes.data if want_curves else None))
        return apk, prec, rcl

    def eval_apk_device(self, gt_offset, gt_points, gt_scale, thresh: float, d_payload_ptr: int, capacity: int, frame_offset: int,
                        d_apk_ptr: int, d_prec_ptr: Optional[int], d_rec_ptr: Optional[int], d_status_ptr: int) -> None:
        """pbd_eval_apk_device: a device payload in, double[nparts] at d_apk_ptr, unless None double[nparts][capacity] at
        d_prec_ptr / d_rec_ptr, the record count (or -1) at d_status_ptr; asynchronous"""
        off, gt, sc = self._apk_args(gt_offset, gt_points, gt_scale)
        self.check(self.lib.pbd_eval_apk_device(self.h, len(off) - 1, off.ctypes.data, gt.ctypes.data, sc.ctypes.data, float(thresh),
                                                d_payload_ptr, capacity, frame_offset, d_apk_ptr, d_prec_ptr, d_rec_ptr, d_status_ptr))

    @staticmethod
    def _cluster_args(deffeat, parent, K):
        d = np.ascontiguousarray(deffeat, np.float64)
        pa = np.ascontiguousarray(parent, np.int32).ravel()
        k = np.ascontiguousarray(K, np.int32).ravel()
        if d.ndim != 3 or d.shape[2] != 2 or len(pa) != d.shape[0] or len(k) != d.shape[0]:
            raise PbdError(-1, "def is (nparts, npos, 2), parent and K (nparts,)")
        return d, pa, k

    def cluster_parts(self, deffeat, parent, K, trials: int = 100, max_iter: int = 1000, seed: int = 0, want_all: bool = True) -> dict:
        """pbd_cluster_parts: clusterparts.m + k_means.m on the device -> {"idx" (nparts, npos), "centres" (nparts, 16, 2),
        "counts" (nparts, 16), "anchors" (nparts, 16, 2), "info" (nparts,) of _lib.CLUSTER_INFO_DTYPE, and with want_all
        "sumdist_all", "iters_all" (nparts, trials)}"""
        d, pa, k = self._cluster_args(deffeat, parent, K)
        P, N, M = d.shape[0], d.shape[1], _lib.MAX_MIX
        out = {"idx": np.zeros((P, N), np.int32), "centres": np.zeros((P, M, 2)), "counts": np.zeros((P, M), np.int32),
               "anchors": np.zeros((P, M, 2), np.int32), "info": np.zeros(P, _lib.CLUSTER_INFO_DTYPE)}
        if want_all:
            out["sumdist_all"] = np.zeros((P, max(int(trials), 0)))
            out["iters_all"] = np.zeros((P, max(int(trials), 0)), np.int32)
        self.check(self.lib.pbd_cluster_parts(self.h, P, N, d.ctypes.data, pa.ctypes.data, k.ctypes.data, int(trials), int(max_iter),
                                              int(seed), out["idx"].ctypes.data, out["centres"].ctypes.data, out["counts"].ctypes.data,
                                              out["anchors"].ctypes.data, out["info"].ctypes.data,
                                              out["sumdist_all"].ctypes.data if want_all else None,
                                              out["iters_all"].ctypes.data if want_all else None))
        return out

    def cluster_parts_device(self, nparts: int, npos: int, d_def_ptr: int, parent, K, trials: int, max_iter: int, seed: int,
                             d_idx_ptr: int, d_centres_ptr: int, d_counts_ptr: int, d_anchors_ptr: int, d_info_ptr: int,
                             d_sumdist_all_ptr: Optional[int] = None, d_iters_all_ptr: Optional[int] = None) -> None:
        """pbd_cluster_parts_device: double[nparts][npos][2] at d_def_ptr in, the outputs of cluster_parts at the device pointers
        (info as {int32, int32, double} records); parent and K are host arrays; asynchronous"""
        pa = np.ascontiguousarray(parent, np.int32).ravel()
        k = np.ascontiguousarray(K, np.int32).ravel()
        if len(pa) != nparts or len(k) != nparts:
            raise PbdError(-1, "parent and K are (nparts,)")
        self.check(self.lib.pbd_cluster_parts_device(self.h, nparts, npos, d_def_ptr, pa.ctypes.data, k.ctypes.data, int(trials),
                                                     int(max_iter), int(seed), d_idx_ptr, d_centres_ptr, d_counts_ptr, d_anchors_ptr,
                                                     d_info_ptr, d_sumdist_all_ptr, d_iters_all_ptr))

    def boxes3d_camera(self, depths: Sequence[np.ndarray], im_shapes, cameras, records: np.ndarray, parts_mode: int = 0,
                       frame_offset: int = 0):
        """pbd_boxes3d_camera: camera boxes (n, 6) float64, part centres (n, max_parts, 3) float32 (0 past ncentres), ncentres (n,)
        and dense (n,) int32 of the records (n, stride); depths[f] float32 2-D, cameras[f] with fx, fy, cx, cy, tx, ty."""
        ds, descs, code = _lib.depth_frames(depths)
        _, _, ir, ic = _lib.shape_arrays(im_shapes)
        rec, ptr = self._records(records), _lib.opt_ptr
        n = len(rec)
        box = np.zeros((n, 6))
        cen = np.zeros((n, self.max_parts, 3), np.float32)
        nc = np.zeros(n, np.int32)
        dn = np.zeros(n, np.int32)
        self.check(self.lib.pbd_boxes3d_camera(self.h, len(ds), descs, code, ir, ic, _lib.pinhole_array(cameras), parts_mode, ptr(rec), n,
                                               frame_offset, ptr(box), ptr(cen), ptr(nc), ptr(dn)))
        return box, cen, nc, dn

    def boxes3d_camera_device(self, descs, depth_code: int, im_shapes, cameras, parts_mode: int, d_payload_ptr: int, capacity: int,
                              frame_offset: int, d_box_ptr: int, d_centres_ptr: int, d_ncentres_ptr: int, d_dense_ptr: int) -> None:
        """pbd_boxes3d_camera_device: the records of a device payload, depth frames (device pointer, rows, cols, pitch), device
        outputs of `capacity` records; asynchronous on the handle's stream"""
        _, _, ir, ic = _lib.shape_arrays(im_shapes)
        self.check(self.lib.pbd_boxes3d_camera_device(self.h, len(descs), _lib.frame_array(descs), depth_code, ir, ic,
                                                      _lib.pinhole_array(cameras), parts_mode, d_payload_ptr, capacity, frame_offset,
                                                      d_box_ptr, d_centres_ptr, d_ncentres_ptr, d_dense_ptr))

    def candidate_mask(self, im_shapes, records: np.ndarray, frames: Optional[Sequence[np.ndarray]] = None, frame_offset: int = 0,
                       labels: bool = True, in_place: bool = False):
        """pbd_candidate_mask: (labels, masked) of the records (n, stride) grouped by ascending frame; im_shapes[f] = (rows, cols) of
        frame index f.  labels: uint8 (rows, cols) per frame (None when labels=False); masked: with `frames` (uint8 (rows, cols) or
        (rows, cols, 1 | 3 | 4), any row pitch), each frame & (label != 0), written over the frames themselves when in_place."""
        ir, ic, pr, pc = _lib.shape_arrays(im_shapes)
        nf = len(ir)
        rec = self._records(records)
        labs = [np.zeros((int(ir[f]), int(ic[f])), np.uint8) for f in range(nf)] if labels else None
        lab_p = (C.c_void_p * nf)(*[a.ctypes.data for a in labs]) if labels else None
        lab_s = (C.c_size_t * nf)(*[a.strides[0] for a in labs]) if labels else None
        cn, col_p, col_s, out_p, out_s, outs = 0, None, None, None, None, None
        if frames is not None:
            if any(f.dtype != np.uint8 or f.strides[-1] != 1 or (f.ndim == 3 and f.strides[1] != f.shape[2]) for f in frames):
                raise PbdError(-1, "frames are uint8 (rows, cols[, channels]) with interleaved channels")
            cn = frames[0].shape[2] if frames[0].ndim == 3 else 1
            outs = list(frames) if in_place else [np.zeros_like(f) for f in frames]
            col_p = (C.c_void_p * nf)(*[f.ctypes.data for f in frames])
            col_s = (C.c_size_t * nf)(*[f.strides[0] for f in frames])
            out_p = (C.c_void_p * nf)(*[f.ctypes.data for f in outs])
            out_s = (C.c_size_t * nf)(*[f.strides[0] for f in outs])
        self.check(self.lib.pbd_candidate_mask(self.h, nf, pr, pc, _lib.opt_ptr(rec), len(rec), frame_offset, lab_p, lab_s, cn, col_p,
                                               col_s, out_p, out_s))
        return labs, outs

    def candidate_mask_device(self, im_shapes, d_payload_ptr: int, capacity: int, frame_offset: int, label_descs=None, channels: int = 0,
                              colour_descs=None, masked_descs=None, d_status_ptr: int = 0) -> None:
        """pbd_candidate_mask_device: the records of a device payload; label_descs / colour_descs / masked_descs: (device pointer,
        pitch) per frame, or None to omit that output; the record count or -1 into the int32 at d_status_ptr; asynchronous"""
        ir, _, pr, pc = _lib.shape_arrays(im_shapes)
        nf = len(ir)
        arr = (lambda d, k, t: None if d is None else (t * nf)(*[e[k] for e in d]))
        self.check(self.lib.pbd_candidate_mask_device(self.h, nf, pr, pc, d_payload_ptr, capacity, frame_offset,
                                                      arr(label_descs, 0, C.c_void_p), arr(label_descs, 1, C.c_size_t), channels, arr(colour_descs, 0, C.c_void_p), arr(colour_descs, 1, C.c_size_t),
                                                      arr(masked_descs, 0, C.c_void_p), arr(masked_descs, 1, C.c_size_t), d_status_ptr))

    def part_poses(self, centres: np.ndarray, ncentres: np.ndarray, dense: np.ndarray):
        """pbd_part_poses: (count (n,) int32, position (n, 3), orientation (n, 4) x, y, z, w, eigenvalues (n, 3)) float32 of what
        boxes3d_camera returns: centres (n, max_parts, 3) float32, ncentres (n,), dense (n,)"""
        nc = np.ascontiguousarray(ncentres, np.int32).reshape(-1)
        n = len(nc)
        cen = np.ascontiguousarray(centres, np.float32).reshape(n, self.max_parts, 3)
        dn = np.ascontiguousarray(dense, np.int32).reshape(n)
        cnt = np.zeros(n, np.int32)
        pos = np.zeros((n, 3), np.float32)
        ori = np.zeros((n, 4), np.float32)
        ev = np.zeros((n, 3), np.float32)
        ptr = _lib.opt_ptr
        self.check(self.lib.pbd_part_poses(self.h, n, ptr(cen), ptr(nc), ptr(dn), ptr(cnt), ptr(pos), ptr(ori), ptr(ev)))
        return cnt, pos, ori, ev

    def part_poses_device(self, d_payload_ptr: int, capacity: int, d_centres_ptr: int, d_ncentres_ptr: int, d_dense_ptr: int,
                          d_count_ptr: int, d_position_ptr: int, d_orientation_ptr: int, d_eigenvalues_ptr: int) -> None:
        """pbd_part_poses_device: boxes3d_camera_device's outputs in, per-record poses out (device arrays of `capacity` records);
        asynchronous on the handle's stream"""
        self.check(self.lib.pbd_part_poses_device(self.h, d_payload_ptr, capacity, d_centres_ptr, d_ncentres_ptr, d_dense_ptr,
                                                  d_count_ptr, d_position_ptr, d_orientation_ptr, d_eigenvalues_ptr))

    @staticmethod
    def cloud_desc(cloud: np.ndarray):
        """(pointer, rows, cols, point_stride, row_stride) of a float32 cloud (rows, cols, k) or (n, k), k >= 3, of any strides"""
        if cloud.dtype != np.float32 or cloud.ndim not in (2, 3) or cloud.shape[-1] < 3 or cloud.strides[-1] != 4:
            raise PbdError(-1, "a cloud is float32 (rows, cols, k) or (n, k) with k >= 3 and the floats of a point contiguous")
        if cloud.ndim == 2:
            return cloud.ctypes.data, 1, cloud.shape[0], cloud.strides[0], cloud.shape[0] * cloud.strides[0]
        return cloud.ctypes.data, cloud.shape[0], cloud.shape[1], cloud.strides[1], cloud.strides[0]

    def cluster_objects(self, clouds: Sequence[np.ndarray], boxes: np.ndarray, frames, index_capacity: Optional[int] = None):
        """pbd_cluster_objects: (centres (n, 3) float32, counts (n,) int32, indices int32 (the kept clusters, box after box)).
        With index_capacity below the total: PbdError PBD_ERR_CAPACITY; its `needed` attribute holds the total."""
        descs = _lib.cloud_array([self.cloud_desc(c) for c in clouds])
        bx = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        n = len(bx)
        if len(fr) != n:
            raise PbdError(-1, "one frame per box")
        cap = sum(c.shape[0] * (c.shape[1] if c.ndim == 3 else 1) for c in clouds) * max(n, 1) if index_capacity is None else index_capacity
        cap = min(cap, 2 ** 31 - 1)
        cen = np.zeros((n, 3), np.float32)
        cnt = np.zeros(n, np.int32)
        need = C.c_int()
        idx = np.zeros(max(min(cap, 1 << 22), 1) if index_capacity is None else max(cap, 1), np.int32)
        rc = self.lib.pbd_cluster_objects(self.h, len(clouds), descs, _lib.opt_ptr(bx), _lib.opt_ptr(fr), n, _lib.opt_ptr(cen),
                                          _lib.opt_ptr(cnt), idx.ctypes.data, len(idx) if index_capacity is None else cap, C.byref(need))
        if rc == -4 and index_capacity is None:          # our own guess was short: once more with the total
            idx = np.zeros(max(need.value, 1), np.int32)
            rc = self.lib.pbd_cluster_objects(self.h, len(clouds), descs, bx.ctypes.data, fr.ctypes.data, n, cen.ctypes.data,
                                              cnt.ctypes.data, idx.ctypes.data, len(idx), C.byref(need))
        if rc != 0:
            err = PbdError(rc, self.lib.pbd_last_error(self.h).decode())
            err.needed = need.value
            raise err
        return cen, cnt, idx[:need.value].copy()

    def cluster_objects_device(self, cloud_descs, d_payload_ptr: int, capacity: int, frame_offset: int, d_boxes_ptr: int,
                               crop_capacity: int, index_capacity: int, d_centres_ptr: int, d_counts_ptr: int, d_indices_ptr: int,
                               d_status_ptr: int) -> None:
        """pbd_cluster_objects_device: device clouds ((pointer, rows, cols, point_stride, row_stride) tuples), the boxes' frames from
        the payload, device boxes / outputs; status int64[2] = {cropped points, output indices or -1}; asynchronous"""
        self.check(self.lib.pbd_cluster_objects_device(self.h, len(cloud_descs), _lib.cloud_array(cloud_descs), d_payload_ptr, capacity,
                                                       frame_offset, d_boxes_ptr, crop_capacity, index_capacity, d_centres_ptr,
                                                       d_counts_ptr, d_indices_ptr, d_status_ptr))

    def remove_planes(self, clouds: Sequence[np.ndarray], params=None, plane_capacity: Optional[int] = None):
        """pbd_remove_planes on organized float32 clouds (rows, cols, k): per cloud (reduced cloud (nkept, 3) float32, kept
        indices int32, labels (rows, cols) int32, planes (nplanes, 4) float32, inliers (nplanes,) int32).  With plane_capacity
        below a cloud's plane count: PbdError PBD_ERR_CAPACITY; its `needed` attribute holds the count."""
        for c in clouds:
            if c.ndim != 3:
                raise PbdError(-1, "pbd_remove_planes takes organized clouds (rows, cols, k)")
        descs = _lib.cloud_array([self.cloud_desc(c) for c in clouds])
        sizes = [c.shape[0] * c.shape[1] for c in clouds]
        total = sum(sizes)
        nc = len(clouds)
        pts = np.zeros((max(total, 1), 3), np.float32)
        kept = np.zeros(max(total, 1), np.int32)
        labels = np.zeros(max(total, 1), np.int32)
        nkept = np.zeros(max(nc, 1), np.int32)
        nplanes = np.zeros(max(nc, 1), np.int32)
        need = C.c_int()

        def run(cap):
            planes = np.zeros((max(nc * cap, 1), 4), np.float32)
            inl = np.zeros(max(nc * cap, 1), np.int32)
            rc = self.lib.pbd_remove_planes(self.h, nc, descs, _lib.plane_params(params), pts.ctypes.data, kept.ctypes.data,
                                            nkept.ctypes.data, labels.ctypes.data, planes.ctypes.data, inl.ctypes.data,
                                            nplanes.ctypes.data, cap, C.byref(need))
            return rc, planes, inl

        cap = 64 if plane_capacity is None else plane_capacity
        rc, planes, inl = run(cap)
        if rc == -4 and plane_capacity is None:          # our own guess was short: once more with the count
            cap = need.value
            rc, planes, inl = run(cap)
        if rc != 0:
            err = PbdError(rc, self.lib.pbd_last_error(self.h).decode())
            err.needed = need.value
            raise err
        out, base = [], 0
        for i, c in enumerate(clouds):
            n, k, npl = sizes[i], int(nkept[i]), int(nplanes[i])
            out.append((pts[base:base + k].copy(), kept[base:base + k].copy(), labels[base:base + n].reshape(c.shape[:2]).copy(),
                        planes[i * cap:i * cap + npl].copy(), inl[i * cap:i * cap + npl].copy()))
            base += n
        return out

    def remove_planes_device(self, cloud_descs, params, d_points_ptr: int, d_kept_ptr: int, d_nkept_ptr: int, d_labels_ptr: int,
                             d_planes_ptr: int, d_inliers_ptr: int, d_nplanes_ptr: int, plane_capacity: int, d_status_ptr: int) -> None:
        """pbd_remove_planes_device: device clouds ((pointer, rows, cols, point_stride, row_stride) tuples), device outputs;
        status int64[2] = {kept points, the most planes of one cloud}; asynchronous"""
        self.check(self.lib.pbd_remove_planes_device(self.h, len(cloud_descs), _lib.cloud_array(cloud_descs), _lib.plane_params(params),
                                                     d_points_ptr, d_kept_ptr, d_nkept_ptr, d_labels_ptr, d_planes_ptr, d_inliers_ptr,
                                                     d_nplanes_ptr, plane_capacity, d_status_ptr))

    def profile(self, on=True):
        """on: False / 0 off, True / 1 every kernel, 2 the convolution only (pbd_profile_enable)"""
        self.check(self.lib.pbd_profile_enable(self.h, int(on)))
        self.check(self.lib.pbd_profile_reset(self.h))

    def profile_read(self):
        out = {}
        for k, name in enumerate(_lib.KERNELS + _lib.KERNELS_MM + _lib.KERNELS_SCALE_NMS):
            ms, n = C.c_double(), C.c_int()
            self.check(self.lib.pbd_profile_read(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def get_stage(self, stage: int, frame: int, level: int, rows: int, cols: int):
        """pbd_get_stage: one stage of one level of the resident result.  After detect_latent it is the latent run's, whose
        responses have one plane per (component, part, mixture) where a detect call's have one per filter: the library refuses a
        buffer sized for the filters then, and the read is made again with one sized for the mixtures."""
        nc, totmix = self.flat.ncomponents, int(self.flat.mix_offset[-1])
        shapes = {_lib.STAGE_FEATURES: [((rows, cols * self.flat.flen), self.dtype)],
                  _lib.STAGE_RESPONSES: [((n, rows, cols), self.dtype) for n in sorted({self.flat.nfilters, totmix})],
                  _lib.STAGE_ROOTV: [((nc, rows, cols), self.dtype)], _lib.STAGE_ROOTI: [((nc, rows, cols), np.int32)]}[stage]
        for k, (shape, dtype) in enumerate(shapes):
            dst = np.empty(shape, dtype)
            rc = self.lib.pbd_get_stage(self.h, stage, frame, level, dst.ctypes.data, dst.nbytes)
            if rc == _lib.PBD_OK or k + 1 == len(shapes) or b"destination holds" not in self.lib.pbd_last_error(self.h):
                self.check(rc)
                return dst

    # ---- the stages and the detect family, as the classes below call them: arguments prepared, one library call each ----------
    def features_pyramid(self, im: np.ndarray, feats: Sequence[np.ndarray]) -> None:
        """pbd_features_pyramid: one HWC image with contiguous pixels (any row pitch), the levels' maps into `feats`"""
        rows, cols, cn = im.shape
        self.check(self.lib.pbd_features_pyramid(self.h, im.ctypes.data, rows, cols, cn, im.strides[0], _lib.DEPTH_CODE[im.dtype],
                                                 _lib.ptr_array(feats)))

    def get_pyramid_image(self, frame: int, level: int, img: np.ndarray) -> None:
        self.check(self.lib.pbd_get_pyramid_image(self.h, frame, level, img.ctypes.data))

    def conv_set_filters(self, filters: Sequence[np.ndarray]) -> None:
        ks = np.array([f.shape[0] for f in filters], np.int32)
        self.check(self.lib.pbd_conv_set_filters(self.h, len(filters), _lib.ptr_array(filters), _lib.ptr(ks, C.c_int)))

    def conv_pdf(self, feats, shapes, resp) -> None:
        """pbd_conv_pdf: shapes[level] = (rows, cols) in cells"""
        _, _, rows, cols = _lib.shape_arrays(shapes)
        self.check(self.lib.pbd_conv_pdf(self.h, len(feats), _lib.ptr_array(feats), rows, cols, _lib.ptr_array(resp)))

    def dp_min(self, scores, shapes, *outs) -> None:
        """pbd_dp_min: outs = Ix, Iy, Ik, rootv, rooti, each a list of one array per level"""
        _, _, rows, cols = _lib.shape_arrays(shapes)
        self.check(self.lib.pbd_dp_min(self.h, len(scores), rows, cols, _lib.ptr_array(scores), *[_lib.ptr_array(o) for o in outs]))
        self.level_shapes = [(int(r), int(c)) for r, c in shapes]

    def dp_argmin(self, scales, capacity: Optional[int] = None) -> List[Candidate]:
        """pbd_dp_argmin; capacity 0 is a capacity: nothing fits, PBD_ERR_CAPACITY"""
        sc = np.ascontiguousarray(scales, np.float32)
        return self._host_list(self.lib.pbd_dp_argmin, (_lib.ptr(sc, C.c_float),), capacity)

    # the detect calls take capacity None or 0 as max_candidates
    def detect(self, im: np.ndarray, capacity: Optional[int] = None) -> List[Candidate]:
        """pbd_detect (uint8) / pbd_detect_typed: one HWC image with contiguous pixels (any row pitch)"""
        args = (im.ctypes.data, im.shape[0], im.shape[1], im.shape[2], im.strides[0])
        if im.dtype == np.uint8:
            return self._host_list(self.lib.pbd_detect, args, capacity or None)
        return self._host_list(self.lib.pbd_detect_typed, args + (_lib.DEPTH_CODE[im.dtype],), capacity or None)

    def detect_batch(self, frames: Sequence[np.ndarray], capacity: Optional[int] = None) -> List[Candidate]:
        """pbd_detect_batch: dense uint8 HWC frames of one shape"""
        rows, cols, cn = frames[0].shape
        return self._host_list(self.lib.pbd_detect_batch, (len(frames), _lib.ptr_array(frames), rows, cols, cn, cols * cn), capacity or None)

    def submit_batch(self, frames: Sequence[np.ndarray]) -> None:
        """pbd_detect_batch_submit: dense uint8 HWC frames of one shape"""
        rows, cols, cn = frames[0].shape
        self.check(self.lib.pbd_detect_batch_submit(self.h, len(frames), _lib.ptr_array(frames), rows, cols, cn, cols * cn))

    def wait_batch(self, capacity: Optional[int] = None, raw: bool = False):
        return self._host_list(self.lib.pbd_detect_batch_wait, (), capacity or None, raw, cached=True)

    def submit_batch_device(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int) -> None:
        self.check(self.lib.pbd_detect_batch_device_submit(self.h, nframes, d_frames_ptr, rows, cols, cn))

    def detect_batch_device(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int, capacity: Optional[int] = None,
                            raw: bool = False):
        return self._host_list(self.lib.pbd_detect_batch_device, (nframes, d_frames_ptr, rows, cols, cn), capacity or None, raw, cached=True)

    def detect_batch_device_out(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int, frame_offset: int,
                                d_payload_ptr: int, capacity: int) -> None:
        self.check(self.lib.pbd_detect_batch_device_out(self.h, nframes, d_frames_ptr, rows, cols, cn, frame_offset, d_payload_ptr, capacity))

    def argmin_device_out(self, frame_offset: int, d_payload_ptr: int, capacity: int) -> None:
        self.check(self.lib.pbd_argmin_device_out(self.h, frame_offset, d_payload_ptr, capacity))

    def detect_frames(self, descs, cn: int, depth_code: int, capacity: Optional[int] = None, device: bool = False) -> List[Candidate]:
        """pbd_detect_frames (host frames) / pbd_detect_frames_device of a pbd_frame[]"""
        fn = self.lib.pbd_detect_frames_device if device else self.lib.pbd_detect_frames
        return self._host_list(fn, (len(descs), descs, cn, depth_code), capacity or None)

    def detect_frames_device_out(self, descs, cn: int, depth_code: int, frame_offset: int, d_payload_ptr: int, capacity: int) -> None:
        """pbd_detect_frames_device_out: frames (device pointer, rows, cols, pitch) of any sizes, the candidate list left on the
        device as detect_batch_device_out leaves it; asynchronous on the handle's stream"""
        self.check(self.lib.pbd_detect_frames_device_out(self.h, len(descs), _lib.frame_array(descs), cn, depth_code, frame_offset,
                                                         d_payload_ptr, capacity))


class HOGFeatures:
    """IFeatures (include/IFeatures.hpp:49-73) as implemented by HOGFeatures<float>."""

    def __init__(self, handle: Handle):
        self.hd = handle
        self._scales = np.zeros(0, np.float32)

    def binsize(self) -> int:
        return self.hd.binsize()

    def nscales(self) -> int:
        return len(self._scales)

    def scales(self) -> np.ndarray:
        return self._scales

    def pyramid(self, im: np.ndarray) -> List[np.ndarray]:
        """pyramid(im, pyrafeatures): list of (H, W*flen) maps of T, fine to coarse."""
        (im,), _, _, _ = _lib.image_frames([im], bad_dtype=-2)     # 8U / 16U / 32F / 64F, anything else is CV_StsUnsupportedFormat
        plan = self.hd.plan(im.shape[0], im.shape[1])
        feats = [np.empty((int(r), int(c) * self.hd.flat.flen), self.hd.dtype) for r, c in zip(plan["feat_rows"], plan["feat_cols"])]
        self.hd.features_pyramid(im, feats)
        self._scales = plan["scales"]
        return feats

    def level_images(self, rows: int, cols: int, cn: int, dtype=np.uint8) -> List[np.ndarray]:
        """the resampled pyramid images of the last pyramid()/detect() call (frame 0), for tests"""
        plan = self.hd.plan(rows, cols)
        out = []
        for l in range(plan["nlevels"]):
            img = np.empty((int(plan["img_rows"][l]), int(plan["img_cols"][l]), cn), dtype)
            self.hd.get_pyramid_image(0, l, img)
            out.append(img)
        return out


class SpatialConvolutionEngine:
    """IConvolutionEngine (include/IConvolutionEngine.hpp:44-68)."""

    def __init__(self, handle: Handle):
        self.hd = handle

    def setFilters(self, filters: Sequence[np.ndarray]) -> None:
        fl = [np.ascontiguousarray(f, self.hd.dtype) for f in filters]
        self.hd.conv_set_filters(fl)
        self._nfilters = len(fl)

    def pdf(self, features: Sequence[np.ndarray]) -> List[np.ndarray]:
        """pdf(features, responses): responses[level] is (nfilters, H, W); responses[level][filter] as in the reference."""
        flen = self.hd.flat.flen
        feats = [np.ascontiguousarray(f, self.hd.dtype) for f in features]
        shapes = [(f.shape[0], f.shape[1] // flen) for f in feats]
        nf = getattr(self, "_nfilters", self.hd.flat.nfilters)
        resp = [np.empty((nf, r, c), self.hd.dtype) for r, c in shapes]
        self.hd.conv_pdf(feats, shapes, resp)
        return resp


class DynamicProgram:
    """DynamicProgram<float> (include/DynamicProgram.hpp:74-75)."""

    def __init__(self, handle: Handle):
        self.hd = handle

    def min(self, scores: Sequence[np.ndarray]):
        """min(parts, scores, Ix, Iy, Ik, rootv, rooti); scores[level] is (nfilters, H, W).
        Returns per level: Ix, Iy, Ik as (nslots, H, W) int32 (slot = pbd_ptr_slot(c, part) + parent mixture),
        rootv (ncomponents, H, W) float32, rooti (ncomponents, H, W) int32."""
        sc = [np.ascontiguousarray(s, self.hd.dtype) for s in scores]
        shapes = [s.shape[1:] for s in sc]
        ns, nc = max(self.hd.flat.nslots, 1), self.hd.flat.ncomponents
        Ix, Iy, Ik = ([np.zeros((ns, r, c), np.int32) for r, c in shapes] for _ in range(3))
        rootv = [np.empty((nc, r, c), self.hd.dtype) for r, c in shapes]
        rooti = [np.empty((nc, r, c), np.int32) for r, c in shapes]
        self.hd.dp_min(sc, shapes, Ix, Iy, Ik, rootv, rooti)
        return Ix, Iy, Ik, rootv, rooti

    def argmin(self, scales: np.ndarray, capacity: Optional[int] = None) -> List[Candidate]:
        """argmin(parts, rootv, rooti, scales, Ix, Iy, Ik, candidates) on the result of the last min()."""
        return self.hd.dp_argmin(scales, capacity)


def _dense_batch(frames: Sequence[np.ndarray]) -> List[np.ndarray]:
    """the frames of a pbd_detect_batch* call: dense uint8 HWC arrays of one shape (the call takes one pitch for all of them)"""
    fr = [np.ascontiguousarray(_lib.hwc(f), np.uint8) for f in frames]
    assert all(f.shape == fr[0].shape for f in fr), "a batch holds equally sized frames"
    return fr


def kept_subsequence(items: Sequence, records: np.ndarray, kept: np.ndarray) -> list:
    """the items whose records a filter kept: `kept` is a subsequence of `records` (items[i]'s is records[i]), matched in order,
    each kept record to the earliest input record equal to it that is still free"""
    keep, k = [], 0
    for item, r in zip(items, records):
        if k < len(kept) and np.array_equal(kept[k], r):
            keep.append(item)
            k += 1
    return keep


class PartsBasedDetector:
    """PartsBasedDetector<float> (include/PartsBasedDetector.hpp:152-175)."""

    def __init__(self, device: int = 0, conv_mode: int = _lib.CONV_EXACT, max_batch: int = 1,
                 max_candidates: int = 1 << 18, stream: Optional[int] = None, dtype=np.float32, nms: Optional[float] = None,
                 remove_planes: bool = False):
        """dtype: the reference's template parameter T (float32 as src/demo.cpp:85, float64 as the ECTO/ROS callers).
        nms: overlap of the per-frame sort + non-maxima suppression run on the device after every detect (Handle.set_nms;
        the callers' post-step, 0.1 in cells/detect.cpp:238 -- config.max_overlap); None: the raw candidate list.
        remove_planes: what clusterObjects does when not told (config.DetectorConfig.remove_planes; fromConfig sets it)."""
        self._kw = dict(device=device, conv_mode=conv_mode, max_batch=max_batch, max_candidates=max_candidates,
                        stream=stream, real_type=_lib.REAL_F32 if np.dtype(dtype) == np.float32 else _lib.REAL_F64)
        self._nms = nms
        self._walk = "reference"
        self._pad = (0, 0)                         # setPadding: off
        self._fine = False                         # setFineOctave: off
        self._root_nms = 0                         # setRootNMS: off
        self._top_k = 0                            # setTopK: off
        self._scale_nms: Optional[int] = None      # setScaleNMS: off
        self._zfactor: Optional[float] = None      # setDepthConsistency: off
        self._dprune: Optional[Tuple[float, float, float]] = None   # setDepthPrune: off
        self.remove_planes = bool(remove_planes)   # clusterObjects' default: the callers' remove_planes option
        self.hd: Optional[Handle] = None
        self._name = ""

    def name(self) -> str:
        return self._name

    @classmethod
    def fromConfig(cls, cfg, **kw) -> "PartsBasedDetector":
        """a detector for a parsed .by_parts pipeline (config.DetectorConfig): its remove_planes option makes clusterObjects
        remove the planes first, as the ECTO cell does (cells/detect.cpp:263-273)"""
        return cls(remove_planes=cfg.remove_planes, **kw)

    def distributeModel(self, model: Model) -> None:
        """src/PartsBasedDetector.cpp:102-127: creates the feature / convolution engines and the DP."""
        if self.hd is not None:
            self.hd.close()
        self.hd = Handle(model, **self._kw)
        self._dc_pays = None
        if self._nms is not None:
            self.hd.set_nms(self._nms)
        if self._walk != "reference":
            self.hd.set_walk(self.WALKS[self._walk])
        if self._pad != (0, 0):
            self.hd.set_padding(*self._pad)
        if self._fine:
            self.hd.set_fine_octave(True)
        if self._root_nms:
            self.hd.set_root_nms(self._root_nms)
        if self._top_k:
            self.hd.set_top_k(self._top_k)
        if self._scale_nms is not None:
            self.hd.set_scale_nms(self._scale_nms)
        if self._dprune is not None:
            self.hd.set_depth_prune(*self._dprune)
        self._name = getattr(model, "name", "")
        self.features_ = HOGFeatures(self.hd)
        self.convolution_engine_ = SpatialConvolutionEngine(self.hd)
        self.dp_ = DynamicProgram(self.hd)

    def _need(self):
        if self.hd is None:
            raise PbdError(-5, "detect() before distributeModel()")

    WALKS = {"reference": _lib.WALK_REFERENCE, "argmax": _lib.WALK_ARGMAX}

    def setWalk(self, walk: str) -> None:
        """how a root is walked to its parts from now on (pbd_set_walk; kept across distributeModel): "reference", the reference's
        composed back-pointers (the default), or "argmax", the placement the score was taken at, so that w . x of every example
        equals its score to rounding -- what training needs (detect.m:139-145)"""
        if walk not in self.WALKS:
            raise PbdError(-1, f"walk {walk!r}: 'reference' or 'argmax'")
        if self.hd is not None:
            self.hd.set_walk(self.WALKS[walk])
        self._walk = walk

    def setPadding(self, padx: Optional[int], pady: Optional[int] = None) -> None:
        """the padded pyramid of the Matlab detector from now on (pbd_set_padding; kept across distributeModel and updateModel):
        every feature level grows by padx / pady cells of the boundary occlusion feature on each side, so that roots and parts
        can lie outside the frame (a person cut off by the frame edge); pady None: pady = padx; padx None or 0: off (the
        default).  Model.full_padding() gives the pad of featpyramid.m.  A Candidate's root is then a cell of the padded plane
        (the image cell is root - (padx, pady)); its part boxes are frame coordinates as always.  Not with setDepthPrune, and
        maxMarginals / marginalPoses refuse a padded result"""
        px = int(padx or 0)
        py = px if pady is None else int(pady or 0)
        if not (0 <= px <= 31 and 0 <= py <= 31):
            raise PbdError(-1, f"padding ({px}, {py}): 0..31 cells")
        if (px or py) and self._dprune is not None:
            raise PbdError(-2, "a padded pyramid with depth pruning on (setDepthPrune(None) first)")
        if self.hd is not None:
            self.hd.set_padding(px, py)
        self._pad = (px, py)

    def setFineOctave(self, on: bool) -> None:
        """search an octave above the frame from now on (pbd_set_fine_octave; kept across distributeModel and updateModel): the
        first `interval` pyramid levels are computed a second time at bin size sbin / 2 on the same level images, so that an
        object of half the model's template size is found.  These levels come first: a Candidate's level then indexes the longer
        list (features_.scales() gives its scales).  Needs an even sbin >= 4; off by default"""
        on = bool(on)
        if self.hd is not None:
            self.hd.set_fine_octave(on)
        self._fine = on

    def setRootNMS(self, sz: int) -> None:
        """the reference's commented-out ssp_.nonMaxSuppression(rootv, scales) (src/PartsBasedDetector.cpp:86) from now on
        (pbd_set_root_nms; kept across distributeModel): only the roots that are grid maxima of their plane within a window of sz
        cells are walked and returned; 0: off (the default).  train() / trainmodel() never turn it on: mining needs every violator"""
        if not 0 <= int(sz) <= 32767:
            raise PbdError(-1, f"root NMS window {sz}: 0 (off) or 1..32767")
        if self.hd is not None:
            self.hd.set_root_nms(int(sz))
        self._root_nms = int(sz)

    def gridNMS(self, src: np.ndarray, sz: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
        """nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp) on the device: the uint8 plane of 0 / 255 (pbd_grid_nms)"""
        self._need()
        return self.hd.grid_nms([src], sz, None if mask is None else [mask])[0]

    def setTopK(self, k: int) -> None:
        """at most k detections per frame from now on (pbd_set_top_k; kept across distributeModel): only the k best roots of each
        frame -- by score, ties to the earlier cell in (level, component, y, x) order -- among those the threshold, depth pruning and
        root NMS leave are walked and returned; 0: off (the default).  train() / trainmodel() never turn it on"""
        if not 0 <= int(k) <= 1 << 30:
            raise PbdError(-1, f"top-K {k}: 0 (off) or 1..2^30")
        if self.hd is not None:
            self.hd.set_top_k(int(k))
        self._top_k = int(k)

    def topKCells(self, values: np.ndarray, k: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
        """the uint8 array of 0 / 255 in values' shape: 255 at the k best elements that are not NaN (and not masked out), ties to
        the smaller index, selected on the device (pbd_top_k_cells)"""
        self._need()
        return self.hd.top_k_cells([values], k, None if mask is None else [mask])[0]

    def topK(self, candidates: Sequence[Candidate], k: int) -> List[Candidate]:
        """per frame index the k best candidates by score, ties to the earlier one, in input order, decided on the device
        (pbd_top_k); the candidates are grouped by ascending frame.  Equal to topk.top_k_records_ref."""
        self._need()
        cands = list(candidates)
        if not cands:
            return []
        rec = self.hd.pack_candidates(cands)
        return kept_subsequence(cands, rec, self.hd.top_k(int(rec[:, 0].max()) + 1, k, rec))

    def setScaleNMS(self, dl: Optional[int]) -> None:
        """a root's duplicates on neighbouring pyramid levels and components suppressed from now on (pbd_set_scale_nms; kept across
        distributeModel): of the roots the threshold, depth pruning and root NMS leave, only those are walked and returned that no
        better root within dl levels of the same frame beats -- two roots being neighbours when the centre of one's rectangle lies
        inside the other's.  Top-K is then taken among these scale-space maxima.  dl in 0..255; None: off (the default).
        train() / trainmodel() never turn it on: mining needs every violator"""
        if dl is not None and not 0 <= int(dl) <= 255:
            raise PbdError(-1, f"scale NMS level distance {dl}: None (off) or 0..255")
        if self.hd is not None:
            self.hd.set_scale_nms(None if dl is None else int(dl))
        self._scale_nms = None if dl is None else int(dl)

    def scaleNMS(self, candidates: Sequence[Candidate], dl: int) -> List[Candidate]:
        """per frame index the candidates no better neighbouring candidate within dl levels beats, in input order, decided on the
        device (pbd_scale_nms); the candidates are grouped by ascending frame.  Equal to scalenms.filter_records.  The form for
        the merged lists of level-sharded detectors"""
        self._need()
        cands = list(candidates)
        if not cands:
            return []
        rec = self.hd.pack_candidates(cands)
        return kept_subsequence(cands, rec, self.hd.scale_nms(int(rec[:, 0].max()) + 1, dl, rec))

    def setDepthPrune(self, fx: Optional[float], width: float = 0.0, tol: float = 0.3) -> None:
        """the intent of the reference's commented-out ssp_.filterResponseByDepth (src/PartsBasedDetector.cpp:86-93) from now on
        (pbd_set_depth_prune; kept across distributeModel): a call that is given depth images -- detect(im, depth), depths= of
        detect_batch / detect_frames / submit_batch, depth= of detect_regions -- walks and returns only the roots whose box width
        agrees with the depth under it (depthprune.plausible: fx in pixels, width of the root footprint in depth units, relative
        tolerance tol); fx None: off (the default).  Without depth images nothing is pruned."""
        cfg = None if fx is None else (float(fx), float(width), float(tol))
        if cfg is not None and not (all(math.isfinite(v) for v in cfg) and cfg[0] > 0 and cfg[1] > 0 and cfg[2] >= 0):
            raise PbdError(-1, f"depth prune: fx {fx}, width {width} (finite, > 0), tol {tol} (finite, >= 0)")
        if cfg is not None and self._pad != (0, 0):
            raise PbdError(-2, "depth pruning on a padded pyramid (setPadding(0) first)")
        if self.hd is not None:
            self.hd.set_depth_prune(*(cfg or (None,)))
        self._dprune = cfg

    def _bind(self, depths) -> None:
        """the depth images of the next detect call, when pruning is on and the caller gave any"""
        if self._dprune is not None and depths is not None:
            self.hd.bind_depth([np.asarray(d) for d in depths])

    def depthPrune(self, candidates: Sequence[Candidate], depths, fx: float, width: float, tol: float = 0.3) -> List[Candidate]:
        """the candidates whose root box agrees with the depth under it, in order, decided on the device (pbd_depth_prune).
        depths: the depth image of every frame index the candidates carry (one image for one frame).  Equal to
        depthprune.filter_records."""
        self._need()
        if isinstance(depths, np.ndarray):
            depths = [depths]
        cands = list(candidates)
        if not cands:
            return []
        rec = self.hd.pack_candidates(cands)
        return kept_subsequence(cands, rec, self.hd.depth_prune(list(depths), rec, fx, width, tol))

    def setDepthConsistency(self, zfactor: Optional[float] = 0.03) -> None:
        """detect(im, depth) then runs filterCandidatesByDepth(., depth, zfactor) before the suppression, as the reference's
        commented-out call would (src/PartsBasedDetector.cpp:91-93); None: off (the default, depth ignored)"""
        if zfactor is not None and math.isnan(zfactor):
            raise PbdError(-1, "zfactor is NaN")
        self._zfactor = None if zfactor is None else float(zfactor)

    def filterCandidatesByDepth(self, candidates: Sequence[Candidate], depths, zfactor: float = 0.03) -> List[Candidate]:
        """SearchSpacePruning::filterCandidatesByDepth on the device (pbd_depth_consistency): the candidates whose parts agree in
        depth with their parents, in order.  depths: the depth image of every frame index the candidates carry (one image for one
        frame).  Equal to consistency.filter_records."""
        self._need()
        if isinstance(depths, np.ndarray):
            depths = [depths]
        cands = list(candidates)
        if not cands:
            return []
        rec = self.hd.pack_candidates(cands)
        return kept_subsequence(cands, rec, self.hd.depth_consistency(list(depths), rec, zfactor))

    def suppress(self, candidates: Sequence[Candidate], im_shapes, overlap: float) -> List[Candidate]:
        """Candidate.sort + Candidate.nonMaximaSuppression per frame, on the device (pbd_suppress): candidates grouped by
        ascending frame; im_shapes[f] = (rows, cols) of frame index f (one shape for one frame)"""
        self._need()
        if len(im_shapes) and np.isscalar(im_shapes[0]):
            im_shapes = [im_shapes]
        cands = list(candidates)
        if not cands:
            return []
        kept = self.hd.suppress(list(im_shapes), overlap, self.hd.pack_candidates(cands))
        return self.hd.unpack_candidates(kept.ravel(), len(kept))

    # ---- testing a model: matlab/detection/testmodel.m, testmodel_gtbox.m and matlab/evaluation ----------------------
    def partNMS(self, candidates: Sequence[Candidate], overlap: float = 0.3, max_boxes: int = 1000) -> List[Candidate]:
        """nms.m per frame, on the device (pbd_part_nms): candidates grouped by ascending frame (0, 1, ...); the kept ones, frame
        by frame, in pick order.  Not Candidate.nonMaximaSuppression: see include/pbd.h"""
        self._need()
        cands = list(candidates)
        if not cands:
            return []
        nframes = max(c.frame for c in cands) + 1
        kept = self.hd.part_nms(nframes, overlap, self.hd.pack_candidates(cands), max_boxes)
        return self.hd.unpack_candidates(kept.ravel(), len(kept))

    def bestOverlap(self, candidates: Sequence[Candidate], gtboxes, overlap: float = 0.3) -> List[Optional[Candidate]]:
        """bestoverlap.m per frame, on the device (pbd_best_overlap): per row of gtboxes (x1, y1, x2, y2; NaN: none) the highest
        scoring candidate of that frame whose part-centre hull covers more than `overlap` of the box, or None"""
        self._need()
        rec, found = self.hd.best_overlap(gtboxes, overlap, self.hd.pack_candidates(list(candidates)))
        return self._found(rec, found)

    def _found(self, rec: np.ndarray, found) -> List[Optional[Candidate]]:
        rec = rec.reshape(-1, self.hd.stride)
        return [self.hd.unpack_candidates(rec[f], 1)[0] if found[f] else None for f in range(len(rec))]

    def evalPCK(self, poses: Sequence[Optional[Candidate]], gt_points, scale, thresh: float = 0.5):
        """eval_pck.m on the device (pbd_eval_pck): poses[f] is frame f's candidate or None (bestOverlap's output) -> pck
        (nparts,), dist (nparts, nframes)"""
        self._need()
        found = np.array([c is not None for c in poses], np.int32)
        blank = Candidate(parts=np.zeros((self.hd.eval_nparts(), 4), np.int32), confidence=np.zeros(1, np.float32), component=0)
        rec = self.hd.pack_candidates([c if c is not None else blank for c in poses])
        return self.hd.eval_pck(rec, found, gt_points, scale, thresh)

    def evalAPK(self, candidates: Sequence[Candidate], gt_offset, gt_points, gt_scale, thresh: float = 0.5):
        """eval_apk.m + VOCap.m on the device (pbd_eval_apk) -> apk (nparts,), prec, rec (nparts, n)"""
        self._need()
        return self.hd.eval_apk(self.hd.pack_candidates(list(candidates)), gt_offset, gt_points, gt_scale, thresh)

    def clusterParts(self, deffeat, parent, K, trials: int = 100, max_iter: int = 1000, seed: int = 0) -> dict:
        """clusterparts.m on the device (pbd_cluster_parts): the part types of a flexible-mixtures model by `trials` k-means
        restarts per part over the positives' offsets to the parent, and buildmodel.m's anchors.  deffeat (nparts, npos, 2):
        trainmodel.data_def's output; parent (nparts,): 0-based, root -1; K (nparts,): types per part, 1..16.  The detector's
        model is not read.  -> Handle.cluster_parts' dict"""
        self._need()
        return self.hd.cluster_parts(deffeat, parent, K, trials, max_iter, seed)

    def _unsuppressed_payload(self, frames: Sequence[np.ndarray]):
        """the frames' unsuppressed list (the handle's own suppression off) in a device payload of the detector's; the list
        never reaches the host"""
        import torch
        fr, _, cn, code = _lib.image_frames([np.ascontiguousarray(f) for f in frames])     # dense, as their uploads are
        dev = torch.device("cuda", self._kw["device"])
        d_fr = [torch.from_numpy(f).to(dev) for f in fr]
        torch.cuda.synchronize(dev)
        words = 1 + self.hd.max_candidates * self.hd.stride
        pays = getattr(self, "_ev_pays", None)
        if pays is None or pays[0].numel() != words or pays[0].device != dev:
            pays = self._ev_pays = [torch.empty(words, dtype=torch.int32, device=dev) for _ in range(2)]
        with self._unsuppressed():
            descs = [(t.data_ptr(), f.shape[0], f.shape[1], f.strides[0]) for t, f in zip(d_fr, fr)]
            self.hd.detect_frames_device_out(descs, cn, code, 0, pays[0].data_ptr(), self.hd.max_candidates)
        return pays, d_fr

    @contextlib.contextmanager
    def _unsuppressed(self):
        """the handle's suppression off for the calls inside; gives the overlap it had and has again afterwards (None: off)"""
        overlap = self.hd.nms_overlap
        if overlap is not None:
            self.hd.set_nms(None)
        try:
            yield overlap
        finally:
            if overlap is not None:
                self.hd.set_nms(overlap)

    def _read_payload(self, pay, cap: int, overflow: str):
        """(count, the first min(count, cap) records on the host) of a device payload, once the handle's stream has drained: word 0
        is the count, negative when the list the payload was made from had overflowed (PBD_ERR_CAPACITY with `overflow`)"""
        self.hd.synchronize()
        found = int(pay[0].item())
        if found < 0:
            raise PbdError(-4, overflow)
        return found, pay[1:1 + min(found, cap) * self.hd.stride].cpu().numpy()

    def testModel(self, frames: Sequence[np.ndarray], overlap: float = 0.3, max_boxes: int = 1000) -> List[Candidate]:
        """testmodel.m: detect_fast at the model's threshold, then nms(box, overlap), per frame (nframes <= max_batch).  The
        unsuppressed list stays on the device (pbd_detect_frames_device_out -> pbd_part_nms_device); only the kept records
        reach the host"""
        self._need()
        pays, keep = self._unsuppressed_payload(frames)
        cap = self.hd.max_candidates
        self.hd.part_nms_device(len(frames), overlap, max_boxes, pays[0].data_ptr(), cap, 0, pays[1].data_ptr(), cap)
        kept, buf = self._read_payload(pays[1], cap, f"more than max_candidates ({cap}) candidates were found before the suppression")
        return self.hd.unpack_candidates(buf, kept)

    def testModelGtbox(self, frames: Sequence[np.ndarray], gtboxes, overlap: float = 0.3) -> List[Optional[Candidate]]:
        """testmodel_gtbox.m: detect_fast at the model's threshold, then bestoverlap(box, gtbox, overlap), per frame; gtboxes
        (nframes, 4) x1, y1, x2, y2 (the caller's [min(x) min(y) max(x) max(y)] of the annotated points).  The unsuppressed list
        stays on the device; one record per frame reaches the host"""
        import torch
        self._need()
        pays, keep = self._unsuppressed_payload(frames)
        n = len(frames)
        out = torch.zeros(n * (self.hd.stride + 1), dtype=torch.int32, device=pays[0].device)
        torch.cuda.synchronize(out.device)
        self.hd.best_overlap_device(gtboxes, overlap, pays[0].data_ptr(), self.hd.max_candidates, 0, out.data_ptr(),
                                    out.data_ptr() + 4 * n * self.hd.stride)
        overflow = f"more than max_candidates ({self.hd.max_candidates}) candidates were found"
        found, _ = self._read_payload(pays[0], 0, overflow)       # the count alone: detect's own, of every root it found
        if found > self.hd.max_candidates:
            raise PbdError(-4, overflow)
        host = out.cpu().numpy()
        rec, found = host[:n * self.hd.stride], host[n * self.hd.stride:]
        return self._found(rec, found)

    def _detect_depth(self, im: np.ndarray, depth: np.ndarray, capacity: Optional[int]) -> List[Candidate]:
        """detect(im, depth) with setDepthConsistency on: the unsuppressed list, the filter, then the handle's suppression (if
        any), each on the device, the lists passed in device payloads"""
        import torch
        rows, cols, cn = im.shape
        dev = torch.device("cuda", self._kw["device"])
        d_im = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
        dd = np.ascontiguousarray(depth)
        if dd.dtype not in _lib.DEPTH_CODE or dd.ndim != 2:
            raise PbdError(-1, "the depth image is a 2-D uint8, uint16, float32 or float64 array")
        d_depth = torch.from_numpy(dd).to(dev)
        torch.cuda.synchronize(dev)
        cap = capacity or self.hd.max_candidates
        words = 1 + self.hd.max_candidates * self.hd.stride
        pays = getattr(self, "_dc_pays", None)     # the three payloads live with the detector, allocated once per handle
        if pays is None or pays[0].numel() != words or pays[0].device != dev:
            pays = self._dc_pays = [torch.empty(words, dtype=torch.int32, device=dev) for _ in range(3)]
        with self._unsuppressed() as overlap:
            if self._dprune is not None:           # prune at the roots, then the consistency filter, then the suppression
                self.hd.bind_depth_device([(d_depth.data_ptr(), dd.shape[0], dd.shape[1], dd.strides[0])], _lib.DEPTH_CODE[dd.dtype])
            self.hd.detect_frames_device_out([(d_im.data_ptr(), rows, cols, cols * cn * im.dtype.itemsize)], cn,
                                             _lib.DEPTH_CODE[im.dtype], 0, pays[0].data_ptr(), self.hd.max_candidates)
        self.hd.depth_consistency_device([(d_depth.data_ptr(), dd.shape[0], dd.shape[1], dd.strides[0])], _lib.DEPTH_CODE[dd.dtype],
                                         self._zfactor, pays[0].data_ptr(), self.hd.max_candidates, 0, pays[1].data_ptr(),
                                         self.hd.max_candidates)
        out = pays[1]
        if overlap is not None:
            self.hd.suppress_device([(rows, cols)], overlap, pays[1].data_ptr(), self.hd.max_candidates, 0, pays[2].data_ptr(),
                                    self.hd.max_candidates)
            out = pays[2]
        found, buf = self._read_payload(out, cap, f"more than max_candidates ({self.hd.max_candidates}) candidates were found before the filter")
        self.features_._scales = self.hd.plan(rows, cols)["scales"]
        if found > cap:
            raise PbdError(-4, f"{found} candidates kept, capacity {cap}")
        return self.hd.unpack_candidates(buf, found)

    def detect(self, im: np.ndarray, depth: Optional[np.ndarray] = None, capacity: Optional[int] = None) -> List[Candidate]:
        """detect(im[, depth], candidates).  `depth` is ignored as in the reference (:91-93) unless setDepthConsistency(zfactor)
        is on: then the unsuppressed candidates go through filterCandidatesByDepth(depth, zfactor) and then the suppression of
        the detector's `nms` overlap (if any), in the reference's order, on the device.  depth=None skips the filter
        (the reference's `if (!depth.empty())`).  With setDepthPrune on, `depth` (the frame's rows x cols) also prunes the roots
        before the walk: prune -> consistency filter -> suppression."""
        self._need()
        (im,), _, _, _ = _lib.image_frames([im], bad_dtype=-2)
        if self._zfactor is not None and depth is not None:
            return self._detect_depth(im, depth, capacity)
        self._bind(None if depth is None else [depth])
        out = self.hd.detect(im, capacity)
        self.features_._scales = self._plan_levels(im.shape[0], im.shape[1])["scales"]
        return out

    def _plan_levels(self, rows: int, cols: int) -> dict:
        """the pyramid plan of a rows x cols frame, its levels' shapes noted on the handle for the max-marginals"""
        plan = self.hd.plan(rows, cols)
        self.hd.level_shapes = [(int(r), int(c)) for r, c in zip(plan["feat_rows"], plan["feat_cols"])]
        return plan

    def modelVector(self) -> np.ndarray:
        """the model vector w = [biasw | defw | filters] in T (include/pbd.h pbd_model_vector; Model.to_vector)"""
        self._need()
        return self.hd.model_vector()

    def examples(self, candidates):
        """training examples of candidates of the last detect call (Candidate objects or records (n, stride) int32), on the
        device (pbd_examples): (hdr (n, hdr_words) int32, values (n, values) T).  examples.dot(hdr, values, w) gives w . x,
        examples.densify(hdr, values, len(w)) the dense vectors."""
        self._need()
        return self.hd.examples(self._candidate_records(candidates)[0])

    def _candidate_records(self, candidates):
        if isinstance(candidates, np.ndarray):
            return candidates, []
        cands = list(candidates)
        return (self.hd.pack_candidates(cands) if cands else np.zeros((0, self.hd.stride), np.int32)), cands

    def partScores(self, candidates):
        """the score of each part of candidates of the last detect call (Candidate objects or records (n, stride) int32), on the
        device (pbd_part_scores; the rule: partscores.py): (place (n, max_parts, 3) int32 x, y, mixture of
        every part in its level's map, scores (n, max_parts, 4) T appearance, message, bias, total).  Candidate objects receive
        what the reference's record declares and never fills (include/Candidate.hpp:54-72): `confidence` becomes nparts floats,
        [0] still the score (score() reads it) and [p >= 1] part p's appearance, and `mixtures` the parts' types."""
        self._need()
        rec, cands = self._candidate_records(candidates)
        status, place, scores = self.hd.part_scores(rec)
        for i, c in enumerate(cands):
            n = int(status[i])
            conf = np.zeros(n, np.float32)
            conf[0] = np.float32(c.score())
            conf[1:] = scores[i, 1:n, 0].astype(np.float32)
            c.confidence = conf
            c.mixtures = place[i, :n, 2].copy()
        return place, scores

    # ---- max-marginals (the rule: marginals.py) -------------------------------------------------------
    def _level_shapes(self, shapes=None):
        shapes = self.hd.level_shapes if shapes is None else [(int(r), int(c)) for r, c in shapes]
        if shapes is None:
            raise PbdError(-5, "max-marginals before detect() / detect_batch() / dp_.min(): the level shapes are not known")
        return shapes

    def maxMarginals(self, frame: int = 0, device: bool = False, shapes=None):
        """the max-marginals of every part on one frame of the last detect() / detect_batch() / dp_.min() call (pbd_max_marginals):
        per level an (NJ, H, W) array of T, plane gm = the (part, type) pair's global index, mm[gm][y][x] the score of the best
        configuration with that part of that type at (x, y).  device=True: torch views of the resident block instead of copies,
        valid until the next detect call, min(), model update or maxMarginals().  shapes: the levels' (rows, cols) when the
        result was not computed through this object's detect / min."""
        self._need()
        shapes = self._level_shapes(shapes)
        self.hd.max_marginals(frame)
        if not device:
            return [self.hd.get_marginals(l, _lib.MM_VALUES, r, c) for l, (r, c) in enumerate(shapes)]
        return [self._device_view(self.hd.marginals_device(l), (int(self.hd.flat.mix_offset[-1]), r, c)) for l, (r, c) in enumerate(shapes)]

    def _device_view(self, ptr: int, shape):
        """a torch tensor over device memory the handle owns (nothing is copied)"""
        import torch
        dt = np.dtype(self.hd.dtype)

        class View:
            __cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": dt.str, "data": (int(ptr), False), "version": 2,
                                        "strides": None}
        if 0 in shape or not ptr:
            return torch.empty(tuple(shape), dtype=torch.float32 if dt == np.float32 else torch.float64, device=f"cuda:{self._kw['device']}")
        return torch.as_tensor(View(), device=f"cuda:{self._kw['device']}")

    def marginalPoses(self, seeds, frame_offset: int = 0, scales=None) -> List[Optional[Candidate]]:
        """the poses of seeds (n, 6) int32 {level, component, part, type or -1 for the best at the cell, x, y} decoded from the
        max-marginals held (pbd_marginal_poses): per seed a Candidate whose score is the seed's max-marginal, `mixtures` the
        parts' types and `place` their cells (x, y), or None for a bad seed.  scales: as DynamicProgram.argmin takes them, needed
        after dp_.min(); None: the detect call's own."""
        self._need()
        status, rec, place = self.hd.marginal_poses(seeds, scales, frame_offset)
        out: List[Optional[Candidate]] = []
        for i, st in enumerate(status):
            if st <= 0:
                out.append(None)
                continue
            c = self.hd.unpack_candidates(rec[i], 1)[0]
            c.mixtures = place[i, :st, 2].copy()
            c.place = place[i, :st, :2].copy()
            out.append(c)
        return out

    def nBestPoses(self, part: int, k: int, sz: int = 2, frame: int = 0, component: int = 0, scales=None, shapes=None) -> List[Candidate]:
        """up to k poses that differ at `part` (of `component`): per level the part's max-marginal planes are reduced over its types
        on the device, the grid maxima of the reduced planes within sz cells are kept (pbd_grid_nms_device), the k best of them
        over all levels selected (pbd_top_k_cells_device), and those cells decoded (type -1: the best at the cell).  Sorted by
        score, ties in (level, y, x) order."""
        self._need()
        import torch
        flat = self.hd.flat
        if not 0 <= component < flat.ncomponents or not 0 <= part < int(flat.part_offset[component + 1]) - int(flat.part_offset[component]):
            raise PbdError(-1, f"part {part} of component {component} is not in the model")
        shapes = self._level_shapes(shapes)
        mm = self.maxMarginals(frame, device=True, shapes=shapes)
        gp = int(flat.part_offset[component]) + part
        g0, g1 = int(flat.mix_offset[gp]), int(flat.mix_offset[gp + 1])
        dev = f"cuda:{self._kw['device']}"
        with torch.cuda.stream(torch.cuda.ExternalStream(self.hd.stream_ptr(), device=dev)):
            red = torch.cat([m[g0:g1].amax(0).reshape(-1) for m in mm]) if mm else torch.zeros(0, device=dev)
            red = red.contiguous()
            grid = torch.zeros(red.numel(), dtype=torch.uint8, device=dev)
            keep = torch.zeros(red.numel(), dtype=torch.uint8, device=dev)
            real = _lib.real_code(self.hd.dtype)
            self.hd.grid_nms_device([r for r, _ in shapes], [c for _, c in shapes], real, red.data_ptr(), None, sz, grid.data_ptr())
            self.hd.top_k_cells_device([red.numel()], real, red.data_ptr(), grid.data_ptr(), k, keep.data_ptr())
            idx = torch.nonzero(keep).reshape(-1).cpu().numpy()
        off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])])
        seeds = []
        for i in idx:
            l = int(np.searchsorted(off, i, side="right")) - 1
            y, x = divmod(int(i - off[l]), shapes[l][1])
            seeds.append((l, component, part, -1, x, y))
        poses = [p for p in self.marginalPoses(np.asarray(seeds, np.int32).reshape(-1, 6), 0, scales) if p is not None]
        poses.sort(key=lambda c: -c.score())
        return poses

    def scorePlacements(self, candidates, place):
        """the same four values at placements the caller gives (pbd_score_placements): place (n, max_parts, 3) x, y, mixture,
        place[i][0] the root, in the frame, level and component of candidate i.  Returns (status (n,) int32: the parts, or -1 for
        a placement outside the level's map or a part's mixtures, scores (n, max_parts, 4) T).  Scores a ground-truth pose
        under the current weights."""
        self._need()
        rec, _ = self._candidate_records(candidates)
        return self.hd.score_placements(rec, place)

    def examples_device(self, d_payload_ptr: int, capacity: int, frame_offset: int, d_hdr_ptr: int, d_values_ptr: int) -> None:
        """pbd_examples_device on a device payload (as detect_batch_device_out / detect_frames_device_out leave it)"""
        self._need()
        self.hd.examples_device(d_payload_ptr, capacity, frame_offset, d_hdr_ptr, d_values_ptr)

    def detectLatent(self, frames, part_boxes, overlap: float, mixtures=None):
        """latent positives (matlab/detection/detect.m with a bbox) on the device (pbd_detect_latent): per frame the best-scoring
        candidate whose every part p overlaps part_boxes[f][p] = (x1, y1, x2, y2) (inclusive) by more than `overlap`, with the
        mixtures[f][p] >= 0 fixed.  Returns (candidates, found): one Candidate per frame, found[f] = False when no placement
        passes (its candidate then scores below -5e9).  examples(candidates) afterwards gives the positives' feature vectors."""
        self._need()
        if (isinstance(frames, np.ndarray) or is_device_frame(frames)) and frames.ndim in (2, 3) and \
                (frames.ndim == 2 or frames.shape[2] in (1, 3)):
            frames = [frames]
        frames = list(frames)
        if frames and is_device_frame(frames[0]):   # torch tensors on the device, views of larger images included: read in place
            import torch
            descs, cn, code = device_frames(frames)
            torch.cuda.synchronize(frames[0].device)
            rec, found = self.hd.detect_latent_device(descs, cn, code, part_boxes, overlap, mixtures)
        else:
            rec, found = self.hd.detect_latent(frames, part_boxes, overlap, mixtures)
        return self.hd.unpack_candidates(rec.ravel(), len(rec)), found.astype(bool)

    def augmentFrames(self, frames, jobs):
        """rotated and mirrored copies on the device (pbd_augment_frames_device; the rule is
        augment.rotate_ref): jobs = [(frame, mirror, degrees)], copy i = rotate(mirror(frames[frame])), all in one launch.
        frames: numpy arrays (uploaded once) or torch tensors on the detector's device, one dtype and channel count, any sizes.
        Returns one torch tensor per job on the device, rows x cols x channels (rows x cols for 2-D frames), ready for
        detectLatent, train() and trainmodel()."""
        import torch
        self._need()
        frames = list(frames)
        dev = torch.device("cuda", self._kw["device"])
        d_fr = [f if is_device_frame(f) else torch.from_numpy(np.array(f)).to(dev) for f in frames]   # np.array: writable, contiguous
        jobs = [(int(f), bool(m), float(d)) for f, m, d in jobs]
        if not jobs:
            return []
        descs, cn, code = device_frames(d_fr)
        outs = []
        for f, _, d in jobs:
            if not 0 <= f < len(d_fr):
                raise PbdError(-1, f"frame {f} outside 0..{len(d_fr) - 1}")
            r, c, _ = self.hd.augment_plan(d_fr[f].shape[0], d_fr[f].shape[1], d)
            outs.append(torch.empty((r, c) + tuple(d_fr[f].shape[2:]), dtype=d_fr[f].dtype, device=dev))
        odesc = [(o.data_ptr(), o.shape[0], o.shape[1], o.stride(0) * o.element_size()) for o in outs]
        torch.cuda.synchronize(dev)
        self.hd.augment_frames_device(descs, cn, code, jobs, odesc)
        self.hd.synchronize()
        return outs

    def warpPositives(self, frames, boxes, filter: int = 0, bias: int = 0, skip_small: bool = True):
        """warped positives (matlab/learning/train.m poswarp with warppos.m and qp_poswrite) on the device (pbd_warp_positives):
        boxes (n, 5) = frame, x1, y1, x2, y2 (0-based, inclusive) in `frames`; each is padded by one cell, cropped with edge
        replication, resized to (k + 2) * sbin pixels with the detector's own resampler, and its HOG written as the example
        [bias = 1 | filter block] of filter `filter` (bias -1: the filter block alone).  Returns (hdr (n, hdr_words) int32, values
        (n, values) T, kept (n,) bool); with skip_small a box smaller than the filter's pixels is skipped (hdr[2] = -1).  The
        examples go to QP.add as they are.  Mirrored and rotated copies are augmentFrames' (the loop over these calls is train.train)."""
        self._need()
        if isinstance(frames, np.ndarray) and frames.ndim in (2, 3) and (frames.ndim == 2 or frames.shape[2] in (1, 3)):
            frames = [frames]
        hdr, vals, kept = self.hd.warp_positives(list(frames), boxes, filter, bias, skip_small)
        return hdr, vals, kept.astype(bool)

    def warpPositives_device(self, descs, cn: int, depth_code: int, boxes, filter: int, bias: int, skip_small: bool, id_offset: int,
                             d_payload_ptr: int, capacity: int, d_hdr_ptr: int, d_values_ptr: int) -> None:
        """pbd_warp_positives_device: frames already on the device as (pointer, rows, cols, pitch) -- regions of larger images
        included --, the examples and the payload left on the device for QP.add_device(hd, d_payload, capacity, d_hdr, d_values,
        1, id_base), which gives example i the id {1, id_base + id_offset + i, 0, 0, 0}; asynchronous on the detector's stream"""
        self._need()
        self.hd.warp_positives_device(descs, cn, depth_code, boxes, filter, bias, skip_small, id_offset, d_payload_ptr, capacity,
                                      d_hdr_ptr, d_values_ptr)

    def updateModel(self, w_or_qp) -> None:
        """model = vec2model(qp_w, model) in place (matlab/learning/train.m after qp_opt): the detector's parameters become a model
        vector w (a numpy array in modelVector()'s order, or a torch tensor on the detector's device) or the weights of a training
        QP (QP.apply: nothing passes through the host).  Afterwards the detector equals one given
        distributeModel(model.from_vector(w)); model() returns that model."""
        self._need()
        from .qp import QP
        if isinstance(w_or_qp, QP):
            w_or_qp.apply(self.hd)
            return
        import torch
        if isinstance(w_or_qp, torch.Tensor):
            t = w_or_qp.contiguous()
            if not t.is_cuda or t.dtype not in (torch.float32, torch.float64) or t.numel() != self.hd.model_vector_len():
                raise PbdError(-1, "a float32 / float64 device tensor of model_vector_len values")
            torch.cuda.current_stream(t.device).synchronize()
            self.hd.set_model_vector_device(t.data_ptr(), np.float32 if t.dtype == torch.float32 else np.float64)
            return
        self.hd.set_model_vector(w_or_qp)

    def setThreshold(self, thresh: float) -> None:
        """model.thresh = thresh (train.m: the 5th percentile of qp_scorepos) for every later detect call"""
        self._need()
        self.hd.set_thresh(thresh)

    def model(self) -> Model:
        """the Model the detector holds now (after updateModel / setThreshold: the updated one)"""
        self._need()
        return self.hd.current_model()

    def qp(self, capacity: int, C: float = 0.002, wpos: float = 2.0, **kw):
        """a training QP (include/pbd.h pbd_qp_*) over a device-resident cache of `capacity` examples of this detector's model
        layout; Cpos = C * wpos, Cneg = C; wreg / w0 / noneg / stream as keywords (None: model2vec's defaults).  It outlives the
        detector.  See partsbaseddetector_amd.qp.QP."""
        self._need()
        from .qp import QP
        return QP(self.hd, capacity, C, wpos, **kw)

    def exampleStride(self):
        """(int32 words of an example's header, values of T of an example)"""
        self._need()
        return self.hd.example_stride()

    def boundingBoxes3D(self, candidates: Sequence[Candidate], depths, im_shapes) -> np.ndarray:
        """Candidate::boundingBox3D(im, depth) of every candidate, on the device (pbd_boxes3d): (n, 6) float64 rows
        {x, y, z, height, width, depth} (Rect3d member order).  `depths` / `im_shapes`: the depth image and the colour frame's
        (rows, cols) of every frame index the candidates carry (a single image / shape for one frame).  Equal to
        [c.boundingBox3D(im_shapes[c.frame], depths[c.frame]) for c in candidates], bit for bit."""
        self._need()
        if isinstance(depths, np.ndarray):
            depths = [depths]
        if len(im_shapes) and np.isscalar(im_shapes[0]):
            im_shapes = [im_shapes]
        return self.hd.boxes3d(list(depths), list(im_shapes), self.hd.pack_candidates(candidates))

    def computeBoundingBoxes(self, candidates: Sequence[Candidate], depths, im_shapes, cameras, parts_mode: int = _lib.PARTS_LITERAL):
        """PointCloudClusterer::computeBoundingBoxes on the device (pbd_boxes3d_camera): (boxes (n, 6) float64, centres
        (n, max_parts, 3) float32, ncentres (n,) int32, dense (n,) int32), indexed by candidate.  depths (float32), im_shapes and
        cameras (pointcloud.PinholeCamera) per frame index the candidates carry (single values for one frame).  Equal bit for bit
        to pointcloud.PointCloudClusterer.computeBoundingBoxes."""
        self._need()
        if isinstance(depths, np.ndarray):
            depths = [depths]
        if len(im_shapes) and np.isscalar(im_shapes[0]):
            im_shapes = [im_shapes]
        if hasattr(cameras, "fx"):
            cameras = [cameras]
        return self.hd.boxes3d_camera(list(depths), list(im_shapes), list(cameras), self.hd.pack_candidates(candidates), parts_mode)

    def mask(self, candidates: Sequence[Candidate], im_shapes, frames=None, in_place: bool = False):
        """Candidate::mask per frame and the ROS node's masked frame `rgb & (mask != 0)`, on the device (pbd_candidate_mask):
        candidates grouped by ascending frame; im_shapes[f] = (rows, cols) of frame index f (one shape for one frame).  Returns the
        labels (one uint8 (rows, cols) per frame) and, when `frames` (uint8 colour frames of 1, 3 or 4 channels) are given, the
        masked frames (written over `frames` when in_place).  Equal to publish.frame_masks / publish.masked_image."""
        self._need()
        if len(im_shapes) and np.isscalar(im_shapes[0]):
            im_shapes = [im_shapes]
        if isinstance(frames, np.ndarray):
            frames = [frames]
        rec = self.hd.pack_candidates(list(candidates))
        labels, masked = self.hd.candidate_mask(list(im_shapes), rec, None if frames is None else list(frames), in_place=in_place)
        return (labels, masked) if frames is not None else labels

    def partPoses(self, centres: np.ndarray, ncentres: np.ndarray, dense: np.ndarray):
        """messagePoses per candidate on the device (pbd_part_poses), from what computeBoundingBoxes returns: (count (n,) int32 --
        0 for "Centroid not found", position (n, 3), orientation (n, 4) as x, y, z, w, eigenvalues (n, 3) ascending) float32.
        Equal bit for bit to publish.part_poses."""
        self._need()
        return self.hd.part_poses(centres, ncentres, dense)

    def removePlanes(self, cloud, params=None):
        """PointCloudClusterer::organizedMultiplaneSegmentation on the device (pbd_remove_planes): (cloud_no_planes (k, 3) float32,
        kept indices (k,) int64, labels (rows, cols) int32 (plane index or -1), planes (n, 4) float32).  cloud: an organized
        float32 (rows, cols, k) cloud; params: pointcloud.PlaneParams or None (the reference's call).  Equal bit for bit to
        pointcloud.PointCloudClusterer.organizedMultiplaneSegmentation."""
        self._need()
        pts, kept, labels, planes, _ = self.hd.remove_planes([cloud], params)[0]
        return pts, kept.astype(np.int64), labels, planes

    def clusterObjects(self, clouds, boxes, frames=None, remove_planes: Optional[bool] = None):
        """PointCloudClusterer::clusterObjects on the device (pbd_cluster_objects): (centres (n, 3) float32, [ascending point
        indices of each box's kept cluster]).  clouds: float32 (rows, cols, k) or (n, k) per frame; boxes (n, 6) camera boxes;
        frames[i] the cloud of box i (all 0 by default).  Equal to pointcloud.PointCloudClusterer.clusterObjects.
        remove_planes (the callers' option; None: the detector's own, False unless set from config.DetectorConfig.remove_planes):
        the organized clouds go through removePlanes first, as in the reference, and the indices then refer to the reduced
        clouds."""
        self._need()
        if isinstance(clouds, np.ndarray):
            clouds = [clouds]
        if self.remove_planes if remove_planes is None else remove_planes:
            clouds = [r[0] for r in self.hd.remove_planes(list(clouds))]
        boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
        frames = np.zeros(len(boxes), np.int32) if frames is None else np.asarray(frames, np.int32)
        cen, cnt, idx = self.hd.cluster_objects(list(clouds), boxes, frames)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        return cen, [idx[off[i]:off[i + 1]].astype(np.int64) for i in range(len(boxes))]

    def detect_batch(self, frames: Sequence[np.ndarray], capacity: Optional[int] = None, depths=None) -> List[Candidate]:
        """Equally sized frames: pbd_detect_batch (8-bit, as before).  Frames of different sizes: pbd_detect_frames, one
        call, the frames' dtype kept when it is one of the four depths (all frames share dtype and channel count).
        depths: one depth image per frame, for setDepthPrune."""
        self._need()
        if len({tuple(f.shape) for f in frames}) > 1:
            return self.detect_frames(frames, capacity, depths)
        fr = _dense_batch(frames)
        self._bind(depths)
        out = self.hd.detect_batch(fr, capacity)
        self._plan_levels(fr[0].shape[0], fr[0].shape[1])
        return out

    def detect_frames(self, frames: Sequence[np.ndarray], capacity: Optional[int] = None, depths=None) -> List[Candidate]:
        """pbd_detect_frames: frames of any sizes in one call; the records of one detect() per frame, concatenated,
        `frame` = index in the list.  depths: one depth image per frame (its rows x cols), for setDepthPrune."""
        self._need()
        fr, descs, cn, code = _lib.image_frames(frames, bad_dtype=-2)
        self._bind(depths)
        return self.hd.detect_frames(descs, cn, code, capacity)

    def detect_regions(self, image, rects, capacity: Optional[int] = None, depth=None) -> List[Candidate]:
        """Regions (x, y, w, h) of one device image -- a torch uint8 tensor, HWC (or HW), on this detector's device -- in
        one pbd_detect_frames_device call, read in place.  The work is ordered behind torch's current stream.  Each
        candidate carries `frame` = index of its region and `offset` = (x, y) of that region: its boxes are in the region's
        coordinates (as detect(im(roi))), offset them to map into the image.  depth: the image's depth map, a 2-D torch tensor
        (uint8, int16 bits of uint16, float32 or float64) of the image's rows x cols on the same device, for setDepthPrune: every
        region reads its own part of it in place."""
        import torch
        self._need()
        if image.dtype != torch.uint8 or image.device.type != "cuda" or image.dim() not in (2, 3):
            raise PbdError(-1, "detect_regions takes a uint8 HWC (or HW) tensor on the GPU")
        if image.device.index != self._kw["device"]:
            raise PbdError(-1, f"the tensor is on {image.device}, this detector on cuda:{self._kw['device']}")
        H, W = image.shape[0], image.shape[1]
        cn = image.shape[2] if image.dim() == 3 else 1
        if image.stride(-1) != 1 or (image.dim() == 3 and image.stride(1) != cn):
            raise PbdError(-1, "detect_regions needs interleaved pixels (a row may have any pitch)")
        pitch = image.stride(0)
        descs = []
        for (x, y, w, h) in rects:
            if not (0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= W and y + h <= H):
                raise PbdError(-1, f"region {(x, y, w, h)} outside the {W}x{H} image")
            descs.append((image.data_ptr() + y * pitch + x * cn, h, w, pitch))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(image.device))
        torch.cuda.ExternalStream(self.hd.stream_ptr(), device=image.device).wait_event(ev)
        if self._dprune is not None and depth is not None:
            codes = {torch.uint8: 0, torch.int16: 2, torch.float32: 5, torch.float64: 6}
            if depth.dtype not in codes or depth.device != image.device or depth.dim() != 2 or tuple(depth.shape) != (H, W) \
                    or depth.stride(1) != 1:
                raise PbdError(-1, "detect_regions: depth is a 2-D tensor of the image's rows x cols on its device")
            es, dp = depth.element_size(), depth.stride(0) * depth.element_size()
            self.hd.bind_depth_device([(depth.data_ptr() + y * dp + x * es, h, w, dp) for (x, y, w, h) in rects], codes[depth.dtype])
        out = self.hd.detect_frames(_lib.frame_array(descs), cn, 0, capacity, device=True)
        for c in out:
            c.offset = (int(rects[c.frame][0]), int(rects[c.frame][1]))
        return out

    def detect_frames_device_out(self, descs, cn: int, frame_offset: int, d_payload_ptr: int, capacity: int,
                                 depth_code: int = 0) -> None:
        """pbd_detect_frames_device_out: frames (device pointer, rows, cols, pitch) of any sizes, the candidate list left on
        the device as detect_batch_device_out leaves it; asynchronous on the handle's stream"""
        self._need()
        self.hd.detect_frames_device_out(descs, cn, depth_code, frame_offset, d_payload_ptr, capacity)

    def submit_batch(self, frames: Sequence[np.ndarray], depths=None) -> None:
        """pbd_detect_batch_submit: stage + transfer + enqueue the whole path for `frames` without waiting (at most
        two batches in flight); `wait_batch` returns the results in submission order.  depths: one depth image per frame, for
        setDepthPrune (copied before the call returns)."""
        self._need()
        fr = _dense_batch(frames)
        self._bind(depths)
        self.hd.submit_batch(fr)

    def wait_batch(self, capacity: Optional[int] = None, raw: bool = False):
        """pbd_detect_batch_wait: the oldest submitted batch's candidates; raw: (the handle's record buffer, count), valid until
        the next wait_batch / detect_batch_device"""
        self._need()
        return self.hd.wait_batch(capacity, raw)

    @property
    def _buf(self) -> Optional[np.ndarray]:
        """the record buffer wait_batch / detect_batch_device fill and return with raw=True (the handle's, reused)"""
        return self.hd._buf

    def submit_batch_device(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int) -> None:
        """pbd_detect_batch_device_submit: like submit_batch for frames already resident in device memory"""
        self._need()
        self.hd.submit_batch_device(d_frames_ptr, nframes, rows, cols, cn)

    def detect_batch_device_out(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int, frame_offset: int,
                                d_payload_ptr: int, capacity: int) -> None:
        """pbd_detect_batch_device_out: the whole path, candidate list left on the device in int32[1 + capacity*stride]
        ([found | sorted records], frame ids + frame_offset); asynchronous on the handle's stream"""
        self._need()
        self.hd.detect_batch_device_out(d_frames_ptr, nframes, rows, cols, cn, frame_offset, d_payload_ptr, capacity)

    def argmin_device_out(self, frame_offset: int, d_payload_ptr: int, capacity: int) -> None:
        """pbd_argmin_device_out: re-emit the candidate list of the batch still resident on the device (after an overflow)"""
        self._need()
        self.hd.argmin_device_out(frame_offset, d_payload_ptr, capacity)

    def detect_batch_device(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int,
                            capacity: Optional[int] = None, raw: bool = False):
        """frames already resident in device memory (e.g. a torch uint8 tensor's data_ptr())."""
        self._need()
        return self.hd.detect_batch_device(d_frames_ptr, nframes, rows, cols, cn, capacity, raw)


class DetectorPool:
    """K detectors of one model on one GPU -- K handles, i.e. K HIP streams and K workspaces -- fed round-robin.

    A handle runs its kernels in order on its own stream; the kernels of a small batch do not fill the chip (a single frame's
    launches are smaller than the chip).  Batches submitted to DIFFERENT handles overlap at kernel granularity.  Measured on
    MI355X: one 640x480 frame per step 423 -> 525 detections/s with four handles, one 1920x1080 frame 83 -> 103 with three;
    batches that fill the chip (64 x 640x480, 8 x 1920x1080) gain nothing (profiles/r03_bench_*s*.json,
    profiles/r03_streams_*.txt).  Results come back in submission order; every batch is computed by exactly one handle, so
    they are those of a single PartsBasedDetector.  A wait_batch() that raises has consumed its batch: the batches behind it
    on the other lanes stay collectable, in order.

        pool = DetectorPool(model, n=3, max_batch=64)
        for batch in stream:                       # frames resident on the device
            pool.submit_batch_device(ptr, nframes, rows, cols, cn)
            while pool.ready_before_next_submit: handle(pool.wait_batch())
        while pool.pending: handle(pool.wait_batch())
    """

    def __init__(self, model: Model, n: int = 3, **kw):
        """kw: PartsBasedDetector's keywords, for every handle (nms=overlap included)"""
        if n < 1:
            raise ValueError("DetectorPool needs at least one detector")
        self.dets: List[PartsBasedDetector] = []
        try:
            for _ in range(n):
                d = PartsBasedDetector(**kw)
                d.distributeModel(model)
                self.dets.append(d)
        except Exception:           # a later handle failed (e.g. out of memory): release the earlier ones
            self.close()
            raise
        self._submitted = 0         # batches submitted so far
        self._collected = 0         # batches handed back so far

    @property
    def pending(self) -> int:
        return self._submitted - self._collected

    @property
    def ready_before_next_submit(self) -> bool:
        """True when the lane the next submit would use still holds an uncollected batch (collect one first)"""
        return self.pending >= len(self.dets)

    def _lane(self, i: int) -> "PartsBasedDetector":
        return self.dets[i % len(self.dets)]

    def submit_batch_device(self, d_frames_ptr: int, nframes: int, rows: int, cols: int, cn: int) -> None:
        if self.ready_before_next_submit:
            raise PbdError(-5, "DetectorPool: every lane holds an uncollected batch; call wait_batch() first")
        self._lane(self._submitted).submit_batch_device(d_frames_ptr, nframes, rows, cols, cn)
        self._submitted += 1

    def submit_batch(self, frames: Sequence[np.ndarray], depths=None) -> None:
        """depths: one depth image per frame, bound on the lane that takes the batch (setDepthPrune)"""
        if self.ready_before_next_submit:
            raise PbdError(-5, "DetectorPool: every lane holds an uncollected batch; call wait_batch() first")
        self._lane(self._submitted).submit_batch(frames, depths)
        self._submitted += 1

    def wait_batch(self, capacity: Optional[int] = None, raw: bool = False):
        """the oldest uncollected batch's candidates (as PartsBasedDetector.wait_batch).

        A wait that fails -- PbdError(-4): more candidates than `capacity`, or than max_candidates before the suppression --
        has still released its lane's slot (pbd_detect_batch_wait, include/pbd.h), so that batch counts as collected: the
        exception reaches the caller, its records beyond what fitted are gone, and the next wait_batch() returns the NEXT
        batch from the next lane.  Only the pool's own "nothing submitted" refusal leaves the cursor where it was."""
        if not self.pending:
            raise PbdError(-5, "DetectorPool.wait_batch(): nothing submitted")
        lane = self._lane(self._collected)
        self._collected += 1        # whatever the lane call does below: its slot is released, the cursor moves on
        return lane.wait_batch(capacity, raw)

    def setPadding(self, padx: Optional[int], pady: Optional[int] = None) -> None:
        """PartsBasedDetector.setPadding on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setPadding(padx, pady)

    def setFineOctave(self, on: bool) -> None:
        """PartsBasedDetector.setFineOctave on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setFineOctave(on)

    def setRootNMS(self, sz: int) -> None:
        """PartsBasedDetector.setRootNMS on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setRootNMS(sz)

    def setTopK(self, k: int) -> None:
        """PartsBasedDetector.setTopK on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setTopK(k)

    def setScaleNMS(self, dl: Optional[int]) -> None:
        """PartsBasedDetector.setScaleNMS on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setScaleNMS(dl)

    def setDepthPrune(self, fx: Optional[float], width: float = 0.0, tol: float = 0.3) -> None:
        """PartsBasedDetector.setDepthPrune on every lane (no batch may be pending)"""
        for d in self.dets:
            d.setDepthPrune(fx, width, tol)

    def close(self) -> None:
        for d in self.dets:
            if d.hd is not None:
                d.hd.close()
