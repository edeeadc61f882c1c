"""train(): the loop of the reference's matlab/learning/train.m over the device calls (include/pbd.h), and
train_ref(), the same loop in numpy over the CPU oracle, the arg-max yardstick of examples.py, warp.py and QPRef.

One iteration (train.m:73-125): empty the QP; the positives (latent, or warped for a one-part model) become fixed support
vectors; optimise and update the model; mine negatives frame batch by frame batch with a second detector of interval
``neg_interval`` and threshold -1, adding every record as a negative example and its hinge to the upper bound, and re-optimise
when the bounds part or the cache is full (detect.m:133-152); optimise once more; the threshold becomes the 5th percentile of
the positives' scores.

Project decisions: the re-optimisation test runs per batch of negative frames, records enter the cache
in payload order (frame, level, component, y, x; no randperm), a negative is a record with score > -1 (the detector's strict
compare), the mining detector is a second handle, and a reused slot starts at a = 0.  Both walks are the arg-max walk
(pbd_set_walk): a negative constraint must be the violated placement itself.
"""
from __future__ import annotations

import copy
import math
from typing import List, Optional

import numpy as np

from . import _lib
from . import examples as E
from . import warp as W
from .qp import QPRef, ids_of_records

MINE_GAP = 0.05     # detect.m:149: re-optimise when 1 - lb / ub exceeds it
THRESH_QUANTILE = 0.05


# ---- what both loops share ----------------------------------------------------------------------------------------------
def sparselen(hdr_words: int, values: int) -> int:
    """train.m:207-239 from the example strides: 1 + 2 * blocks + values of the longest example"""
    return 1 + 2 * ((hdr_words - 4) // 2) + values


def default_capacity(npos: int, wpos: float, hdr_words: int, values: int) -> int:
    """nmax of train.m:27-46: maxsize = 10 * (wpos + 1) * npos * 4 * sparselen / 1e9 GB clamped to [6, 7.5], then
    round(maxsize * .25e9 / sparselen)"""
    ln = sparselen(hdr_words, values)
    maxsize = min(max(10.0 * (wpos + 1) * npos * 4 * ln / 1e9, 6.0), 7.5)
    return int(W.matlab_round(maxsize * .25e9 / ln))


def mining_model(model, neg_interval: int):
    """train.m:95-96 with detect(im, model, -1, ...): the model at interval neg_interval and threshold -1"""
    m = copy.deepcopy(model)
    m.interval = int(neg_interval)
    m.thresh = -1.0
    return m


def part_boxes(p) -> np.ndarray:
    return np.asarray(p["boxes"], np.int64).reshape(-1, 4)


def too_small(boxes: np.ndarray, kmax: int, sbin: int) -> bool:
    """train.m:170-182: any part box below minsize = prod(model.maxsize * model.sbin) pixels (inclusive area)"""
    area = (boxes[:, 2] - boxes[:, 0] + 1).astype(np.float64) * (boxes[:, 3] - boxes[:, 1] + 1).astype(np.float64)
    return bool(np.any(area < (float(kmax) * sbin) ** 2))


def croppos(im: np.ndarray, boxes: np.ndarray):
    """croppos.m on 0-based inclusive boxes: the union box padded by half its width plus height, Matlab's round, clipped to
    the frame; returns (the crop as a view of im, the boxes shifted into it)"""
    x1, y1, x2, y2 = int(boxes[:, 0].min()), int(boxes[:, 1].min()), int(boxes[:, 2].max()), int(boxes[:, 3].max())
    pad = 0.5 * ((x2 - x1 + 1) + (y2 - y1 + 1))
    cx1 = max(1, W.matlab_round(x1 + 1 - pad)) - 1
    cy1 = max(1, W.matlab_round(y1 + 1 - pad)) - 1
    cx2 = min(im.shape[1], W.matlab_round(x2 + 1 + pad)) - 1
    cy2 = min(im.shape[0], W.matlab_round(y2 + 1 + pad)) - 1
    out = boxes.copy()
    out[:, [0, 2]] -= cx1
    out[:, [1, 3]] -= cy1
    return im[cy1:cy2 + 1, cx1:cx2 + 1], out


def positive_batches(pos, kmax: int, sbin: int, max_batch: int):
    """(skipped indices, batches): a batch is a run of at most max_batch consecutive positives none of which is skipped, so
    that frame f of its call is positive first + f"""
    skipped, batches, run = [], [], []
    for i, p in enumerate(pos):
        if too_small(part_boxes(p), kmax, sbin):
            skipped.append(i)
            if run:
                batches.append(run)
            run = []
            continue
        run.append(i)
        if len(run) == max_batch:
            batches.append(run)
            run = []
    if run:
        batches.append(run)
    return skipped, batches


def wants_opt(lb: float, ub: float, n: int, capacity: int) -> bool:
    """detect.m:148-149"""
    return lb < 0 or 1 - lb / ub > MINE_GAP or n == capacity


def full_opt(lb: float, n: int, capacity: int) -> bool:
    """detect.m:319: qp_opt + qp_prune, else qp_one"""
    return lb < 0 or n == capacity


def threshold_of(scores) -> float:
    """train.m:117-118: r = sort(qp_scorepos); r(ceil(length(r) * .05))"""
    r = np.sort(np.asarray(scores, np.float64))
    return float(np.float32(r[int(math.ceil(THRESH_QUANTILE * len(r))) - 1]))


_frame = _lib.hwc           # rows x cols x channels of a host array or a device tensor (a view)


def _is_device(im) -> bool:
    return hasattr(im, "data_ptr") and bool(getattr(im, "is_cuda", False))


def positives_on_device(pos) -> bool:
    """whether the positives' images are device tensors (all of them, or none)"""
    dev = [_is_device(p["im"]) for p in pos]
    if any(dev) and not all(dev):
        raise ValueError("the positives' images are all host arrays or all device tensors")
    return bool(dev) and dev[0]


def host_positives(pos):
    """the positives with every device tensor copied to a host array (the yardsticks work on host copies)"""
    return [dict(p, im=p["im"].cpu().numpy()) if _is_device(p["im"]) else p for p in pos]


def _new_iteration() -> dict:
    return {"numpositives": [], "skipped": [], "notfound": [], "batches": []}


def _finish(info: dict, its: List[dict]) -> dict:
    info["iterations"] = its
    info.update({k: v for k, v in its[-1].items()})
    return info


# ---- the device loop ----------------------------------------------------------------------------------------------------
def _detect_latent(hd, crops, boxes, overlap, mixtures):
    """pbd_detect_latent on crops that are views of their frames (rows `strides[0]` apart): nothing is copied on the host"""
    return hd.detect_latent(crops, boxes, overlap, mixtures)


def _detect_latent_device(hd, crops, boxes, overlap, mixtures):
    """pbd_detect_latent_device on crops that are views of device tensors: regions read in place, nothing is copied or uploaded"""
    from .detector import device_frames
    descs, cn, code = device_frames(crops)
    return hd.detect_latent_device(descs, cn, code, boxes, overlap, mixtures)


def _mixtures(pos, idx, nparts):
    if not any(pos[i].get("mix") is not None for i in idx):
        return None
    return [np.full(nparts, -1, np.int32) if pos[i].get("mix") is None else np.asarray(pos[i]["mix"], np.int32) for i in idx]


def train(model, pos, neg, warp, iters: int = 1, C: float = 0.002, wpos: float = 2, capacity: Optional[int] = None,
          overlap: float = 0.6, neg_interval: int = 2, neg_batch: int = 1, tol: float = 0.05, max_passes: int = 1000, seed: int = 0,
          dtype=np.float32, device: int = 0, conv_mode: int = _lib.CONV_EXACT):
    """train.m on the device: (the trained Model, info).  pos: [{"im": ndarray or a torch tensor on the device (an augmented
    copy: its crops are read in place, nothing is uploaded again), "boxes": (nparts, 4) int, 0-based inclusive,
    "mix": optional (nparts,)}]; neg: frames of any sizes; warp: 1 for a one-part model (warped positives), 0 for latent
    positives.  capacity None: train.m's nmax, capped by the device's free memory.  info: per iteration ("iterations") and, at
    top level, of the last one: numpositives per component, skipped / notfound positives, per negative batch {first, found,
    taken, dropped, added, branch ("none", "one", "opt+prune"), lb, ub, n, nsv}, and the final lb, ub, n, nsv, passes, thresh.
    Everything runs on one stream; the examples never leave the device."""
    import torch
    from .detector import PartsBasedDetector
    flat = model.flatten()
    nparts = int(flat.part_offset[1] - flat.part_offset[0])
    if warp and (flat.ncomponents != 1 or nparts != 1):
        raise ValueError("warped positives need a one-part model")
    if not pos or not len(neg):
        raise ValueError("positives and negatives are needed")
    kmax, sbin = int(np.max(flat.filter_ksize)), int(flat.sbin)
    hw, vw = E.strides(flat)
    if positives_on_device(pos):
        torch.cuda.synchronize(pos[0]["im"].device)   # whatever made the tensors has finished before this call's stream reads them
    with torch.cuda.device(device):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            if capacity is None:
                per = vw * (5 + np.dtype(dtype).itemsize) + hw * 4 + (2 + 3 * ((hw - 4) // 2)) * 4 + 64 + (8 + 4 * flat.max_parts) * 4
                capacity = max(1, min(default_capacity(len(pos), wpos, hw, vw), int(0.4 * torch.cuda.mem_get_info()[0] / per)))
            capacity = int(capacity)
            max_batch = max(int(neg_batch), min(len(pos), 8), 1)
            kw = dict(device=device, conv_mode=conv_mode, max_batch=max_batch, max_candidates=max(capacity, 1024),
                      stream=stream.cuda_stream, dtype=dtype)
            det, negdet = PartsBasedDetector(**kw), PartsBasedDetector(**kw)
            det.setWalk("argmax")
            negdet.setWalk("argmax")
            det.distributeModel(model)
            negdet.distributeModel(mining_model(model, neg_interval))
            q = det.qp(capacity, C, wpos, stream=stream.cuda_stream)
            try:
                return _train_device(torch, det, negdet, q, flat, pos, neg, warp, iters, capacity, overlap, neg_batch, tol, max_passes,
                                     seed, dtype, kmax, sbin, nparts, max_batch)
            finally:
                q.close()
                negdet.hd.close()
                det.hd.close()


def _train_device(torch, det, negdet, q, flat, pos, neg, warp, iters, capacity, overlap, neg_batch, tol, max_passes, seed, dtype,
                  kmax, sbin, nparts, max_batch):
    stride = det.hd.stride
    hw, vw = det.exampleStride()
    tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    pay = torch.zeros(1 + capacity * stride, dtype=torch.int32, device="cuda")
    hdr = torch.zeros(capacity * hw, dtype=torch.int32, device="cuda")
    vals = torch.zeros(capacity * vw, dtype=tdt, device="cuda")
    up = lambda im: torch.from_numpy(np.ascontiguousarray(_frame(im))).cuda()
    d_neg = [up(im) for im in neg]
    desc = lambda t: (t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * t.element_size())
    on_device = positives_on_device(pos)
    pos_code = _lib.DEPTH_CODE[np.dtype(str(pos[0]["im"].dtype).replace("torch.", ""))]
    calls = 0

    def next_seed():
        nonlocal calls
        calls += 1
        return seed + calls - 1

    def update():
        det.updateModel(q)
        negdet.updateModel(q)

    its = []
    for _ in range(iters):
        it = _new_iteration()
        q.clear()
        # -- positives
        if warp:
            d_pos = [_frame(p["im"]) if on_device else up(p["im"]) for p in pos]
            boxes = np.array([[i, *part_boxes(p)[0]] for i, p in enumerate(pos)], np.int32)
            if len(boxes) > capacity:
                raise ValueError("more positives than the cache holds")
            gm = int(flat.mix_offset[0])
            det.warpPositives_device([desc(t) for t in d_pos], d_pos[0].shape[2], pos_code, boxes, int(flat.filterid[gm]),
                                     int(flat.biasid[gm]), True, 0, pay.data_ptr(), len(boxes),
                                     hdr.data_ptr(), vals.data_ptr())
            q.add_device(det.hd, pay.data_ptr(), len(boxes), hdr.data_ptr(), vals.data_ptr(), 1, 0)
            k = int(flat.filter_ksize[flat.filterid[gm]])
            it["skipped"] = [i for i, p in enumerate(pos) if not W.keeps(part_boxes(p)[0], k, sbin)]
            it["numpositives"] = [q.state()["n"]]
        else:
            it["numpositives"] = [0] * flat.ncomponents
            it["skipped"], batches = positive_batches(pos, kmax, sbin, min(max_batch, capacity))
            for idx in batches:
                cb = [croppos(_frame(pos[i]["im"]), part_boxes(pos[i])) for i in idx]
                rec, found = (_detect_latent_device if on_device else _detect_latent)(det.hd, [c for c, _ in cb], [b for _, b in cb],
                                                                                      overlap, _mixtures(pos, idx, nparts))
                keep = np.nonzero(found)[0]
                it["notfound"] += [idx[f] for f in range(len(idx)) if not found[f]]
                if len(keep) == 0:
                    continue
                host = np.concatenate([[len(keep)], rec[keep].ravel()]).astype(np.int32)
                pay[:len(host)].copy_(torch.from_numpy(host))
                det.examples_device(pay.data_ptr(), len(keep), 0, hdr.data_ptr(), vals.data_ptr())
                q.add_device(det.hd, pay.data_ptr(), len(keep), hdr.data_ptr(), vals.data_ptr(), 1, idx[0])
                for f in keep:
                    it["numpositives"][int(rec[f, 1])] += 1
        # -- the positives are fixed support vectors; a first model
        q.fix()
        q.prune()
        q.opt(tol, max_passes, next_seed())
        update()
        # -- negatives
        for b0 in range(0, len(neg), neg_batch):
            fr = d_neg[b0:b0 + neg_batch]
            n0 = q.state()["n"]
            paycap = max(capacity - n0, 1)
            negdet.detect_frames_device_out([desc(t) for t in fr], fr[0].shape[2], 0, pay.data_ptr(), paycap,
                                            _lib.DEPTH_CODE[np.dtype(_frame(neg[b0]).dtype)])
            negdet.examples_device(pay.data_ptr(), paycap, 0, hdr.data_ptr(), vals.data_ptr())
            q.add_device(negdet.hd, pay.data_ptr(), paycap, hdr.data_ptr(), vals.data_ptr(), -1, b0)
            added = q.add_loss_device(pay.data_ptr(), paycap, -1)
            found = int(pay[0].item())
            st = q.state()
            batch = {"first": b0, "found": found, "taken": st["n"] - n0, "dropped": max(found - (st["n"] - n0), 0), "added": added,
                     "branch": "none"}
            if wants_opt(st["lb"], st["ub"], st["n"], capacity):
                if full_opt(st["lb"], st["n"], capacity):
                    q.opt(tol, max_passes, next_seed())
                    q.prune()
                    batch["branch"] = "opt+prune"
                else:
                    q.one(seed=next_seed())
                    batch["branch"] = "one"
                update()
                st = q.state()
            batch.update(lb=st["lb"], ub=st["ub"], n=st["n"], nsv=st["nsv"])
            it["batches"].append(batch)
            if batch["branch"] != "none" and st["nsv"] == capacity:
                break
        # -- finish
        st = q.opt(tol, max_passes, next_seed())
        update()
        thresh = threshold_of(q.scores())
        det.setThreshold(thresh)
        it.update(lb=st["lb"], ub=st["ub"], n=st["n"], nsv=st["nsv"], passes=st["passes"], thresh=thresh)
        its.append(it)
    return det.model(), _finish({"capacity": capacity}, its)


# ---- the same loop in numpy ---------------------------------------------------------------------------------------------
def _records_of(dets, frame: int, stride: int) -> np.ndarray:
    """oracle.detect's records of one frame as payload records (the header words; the part boxes are not used)"""
    rec = np.zeros((len(dets), stride), np.int32)
    for i, r in enumerate(dets):
        rec[i, :5] = (frame, r["component"], r["level"], r["root_x"], r["root_y"])
        rec[i, 5:6] = np.array([r["score"]], np.float32).view(np.int32)
    return rec


def train_ref(model, pos, neg, warp, iters: int = 1, C: float = 0.002, wpos: float = 2, capacity: Optional[int] = None,
              overlap: float = 0.6, neg_interval: int = 2, neg_batch: int = 1, tol: float = 0.05, max_passes: int = 1000,
              seed: int = 0, dtype=np.float32):
    """train() in numpy: oracle.detect for the negatives (interval neg_interval, threshold -1), latent_search(walk="argmax")
    and warp.warp_examples for the positives, examples_of_records(walk="argmax"), QPRef and Model.from_vector.  The same
    (Model, info); capacity None: train.m's nmax without the device's cap."""
    from oracle import oracle
    pos = host_positives(pos)
    flat = model.flatten()
    nparts = int(flat.part_offset[1] - flat.part_offset[0])
    if warp and (flat.ncomponents != 1 or nparts != 1):
        raise ValueError("warped positives need a one-part model")
    kmax, sbin = int(np.max(flat.filter_ksize)), int(flat.sbin)
    hw, vw = E.strides(flat)
    stride = 8 + 4 * flat.max_parts
    capacity = default_capacity(len(pos), wpos, hw, vw) if capacity is None else int(capacity)
    max_batch = min(max(int(neg_batch), min(len(pos), 8), 1), capacity)
    q = QPRef(flat, capacity, C, wpos)
    calls = 0

    def next_seed():
        nonlocal calls
        calls += 1
        return seed + calls - 1

    def nsv():
        return int(sum(q.sv))

    its = []
    for _ in range(iters):
        it = _new_iteration()
        q.clear()
        flat = model.flatten()
        if warp:
            boxes = np.array([[i, *part_boxes(p)[0]] for i, p in enumerate(pos)], np.int32)
            gm = int(flat.mix_offset[0])
            H, V, kept = W.warp_examples(flat, [_frame(p["im"]) for p in pos], boxes, int(flat.filterid[gm]), int(flat.biasid[gm]),
                                         True, dtype)
            ids = np.zeros((len(boxes), 5), np.int32)
            ids[:, 0], ids[:, 1] = 1, np.arange(len(boxes))
            q.add(H, V, ids)
            it["skipped"] = [int(i) for i in np.nonzero(kept == 0)[0]]
            it["numpositives"] = [q.n]
        else:
            it["numpositives"] = [0] * flat.ncomponents
            it["skipped"], batches = positive_batches(pos, kmax, sbin, max_batch)
            for i in (i for idx in batches for i in idx):
                crop, bx = croppos(_frame(pos[i]["im"]), part_boxes(pos[i]))
                got = E.latent_search(model, crop, bx, overlap, pos[i].get("mix"), dtype, walk="argmax")
                if not got["found"]:
                    it["notfound"].append(i)
                    continue
                feats, _ = oracle.features_pyramid(flat, crop, dtype)
                h, v = E.example(flat, feats[got["level"]], got["component"], got["placement"], 0, dtype)
                q.add(h, v, [[1, i, got["level"], got["root_x"], got["root_y"]]])
                it["numpositives"][got["component"]] += 1
        q.fix()
        q.prune()
        q.opt(tol, max_passes, next_seed())
        model = model.from_vector(q.weights())
        for b0 in range(0, len(neg), neg_batch):
            negflat = mining_model(model, neg_interval).flatten()
            frames = [_frame(im) for im in neg[b0:b0 + neg_batch]]
            n0 = q.n
            paycap = max(capacity - n0, 1)
            rec = np.concatenate([_records_of(oracle.detect(negflat, im, dtype), f, stride) for f, im in enumerate(frames)])
            found, rec = len(rec), rec[:paycap]
            maps = [E.FrameMaps(negflat, im, dtype, walk="argmax") for im in frames]
            H, V = E.examples_of_records(negflat, maps, rec, 0, dtype)
            q.add(H, V, ids_of_records(rec, -1, b0))
            added = q.add_loss(rec, -1)
            batch = {"first": b0, "found": found, "taken": q.n - n0, "dropped": max(found - (q.n - n0), 0), "added": added,
                     "branch": "none"}
            if wants_opt(q.lb, q.ub, q.n, capacity):
                if full_opt(q.lb, q.n, capacity):
                    q.opt(tol, max_passes, next_seed())
                    q.prune()
                    batch["branch"] = "opt+prune"
                else:
                    q.one(seed=next_seed())
                    batch["branch"] = "one"
                model = model.from_vector(q.weights())
            batch.update(lb=q.lb, ub=q.ub, n=q.n, nsv=nsv())
            it["batches"].append(batch)
            if batch["branch"] != "none" and nsv() == capacity:
                break
        q.opt(tol, max_passes, next_seed())
        model = model.from_vector(q.weights())
        thresh = threshold_of(q.scores())
        model.thresh = thresh
        it.update(lb=q.lb, ub=q.ub, n=q.n, nsv=nsv(), passes=q.passes, thresh=thresh)
        its.append(it)
    return model, _finish({"capacity": capacity}, its)
