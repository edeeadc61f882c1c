"""MatlabIOModel: models in the layout the Matlab training code writes (Yang & Ramanan's ``matlab/learning``), read from
and written to level 5 MAT-files (matio.py).  ``deserialize`` does what the reference's MatlabIOModel::deserialize
(src/MatlabIOModel.cpp:66-187) does, conversion for conversion:

- ``name``: the variable ``name``; the file's stem when there is none;
- ``interval`` / ``thresh`` / ``sbin``: ``model.interval`` / ``.thresh`` / ``.sbin`` (int / float / int, truncating);
  ``norient`` is fixed at 18;
- ``filtersw[f]``: ``model.filters(f).w`` (sizy x sizx x C) flattened to (sizy, sizx*C) with ``[m, n*C + c] = w(m, n, c)``;
  ``flen`` is C;
- ``filterid`` / ``defid`` / ``biasid`` / ``parentid``: ``model.components{c}(p).filterid`` / ``.defid`` / ``.biasid`` /
  ``.parent``, 1-based to 0-based; a matrix ``biasid`` is flattened row-major over Matlab's (i, j);
- ``defw[d]``: ``model.defs(d).w`` rounded to float; ``anchors[d]``: ``model.defs(d).anchor`` ``[x y ds]`` as
  ``(x - 1, y - 1)``, x and y truncated to int;
- ``biasw[b]``: ``model.bias(b).w`` rounded to float.

Other fields (``pa``, ``maxsize``, ``len``, ``obj``, the ``.i`` offsets, ...) are ignored; field order does not matter.
``serialize`` writes the same layout (the reference leaves MatlabIOModel::serialize a TODO).
"""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np

from . import matio
from .matio import MatCell, MatStruct
from .model import Model


def _get(elem: Dict, field: str, path: str):
    if field not in elem:
        raise ValueError(f"missing field {path}.{field}")
    return elem[field]


def _structs(v, path: str) -> MatStruct:
    if not isinstance(v, MatStruct):
        raise ValueError(f"{path} is not a struct array")
    return v


def _numeric(v, path: str) -> np.ndarray:
    if not isinstance(v, np.ndarray) or v.dtype.kind not in "biuf":
        raise ValueError(f"{path} is not a numeric array")
    return v.astype(np.float64)


def _scalar(v, path: str) -> float:
    a = _numeric(v, path)
    if a.size < 1:
        raise ValueError(f"{path} is empty")
    return float(a.ravel(order="F")[0])


def _ids(v, path: str) -> List[int]:
    """a 1-based index array, row-major over Matlab's (i, j) (cv::Mat's iteration order), 0-based"""
    return [int(x) - 1 for x in _numeric(v, path).ravel(order="C")]


def deserialize(filename: str) -> Model:
    """MatlabIOModel::deserialize (src/MatlabIOModel.cpp:66-187).  ValueError names a missing or mistyped field by its
    Matlab path, e.g. ``model.components{2}(5).defid``."""
    try:
        return _deserialize(filename)
    except ValueError as e:
        raise ValueError(f"{filename}: {e}") from None


def _deserialize(filename: str) -> Model:
    variables = matio.loadmat(filename)
    if "name" in variables:
        name = variables["name"]
        if not isinstance(name, str):
            raise ValueError("variable name is not a char row")
    else:
        name = os.path.splitext(os.path.basename(filename))[0]
    if "model" not in variables:
        raise ValueError("missing variable model")
    top = _structs(variables["model"], "model")
    if len(top) < 1:
        raise ValueError("model is an empty struct array")
    mdl = top[0]

    m = Model(name=name, norient=18)
    m.interval = int(_scalar(_get(mdl, "interval", "model"), "model.interval"))
    m.thresh = _scalar(_get(mdl, "thresh", "model"), "model.thresh")
    m.sbin = int(_scalar(_get(mdl, "sbin", "model"), "model.sbin"))

    filters = _structs(_get(mdl, "filters", "model"), "model.filters")
    for f in range(len(filters)):
        path = f"model.filters({f + 1})"
        w = _numeric(_get(filters[f], "w", path), path + ".w")
        if w.ndim == 2:
            w = w[:, :, None]
        if w.ndim != 3:
            raise ValueError(f"{path}.w has {w.ndim} dimensions, not 3")
        M, N, C = w.shape
        m.flen = C
        m.filtersw.append(np.ascontiguousarray(w.reshape(M, N * C)))    # [m, n*C + c] = w(m, n, c)

    components = _get(mdl, "components", "model")
    if not isinstance(components, MatCell):
        raise ValueError("model.components is not a cell array")
    for c, comp in enumerate(components):
        cpath = f"model.components{{{c + 1}}}"
        comp = _structs(comp, cpath)
        fid, bid, did, par = [], [], [], []
        for p in range(len(comp)):
            path = f"{cpath}({p + 1})"
            part = comp[p]
            did.append(_ids(_get(part, "defid", path), path + ".defid"))
            fid.append(_ids(_get(part, "filterid", path), path + ".filterid"))
            par.append(int(_scalar(_get(part, "parent", path), path + ".parent")) - 1)
            bid.append(_ids(_get(part, "biasid", path), path + ".biasid"))
        m.filterid.append(fid)
        m.biasid.append(bid)
        m.defid.append(did)
        m.parentid.append(par)

    defs = _structs(_get(mdl, "defs", "model"), "model.defs")
    for d in range(len(defs)):
        path = f"model.defs({d + 1})"
        m.defw.append([float(np.float32(v)) for v in _numeric(_get(defs[d], "w", path), path + ".w").ravel(order="C")])
        a = _numeric(_get(defs[d], "anchor", path), path + ".anchor").ravel(order="C")
        if a.size < 2:
            raise ValueError(f"{path}.anchor has {a.size} elements, not [x y ds]")
        m.anchors.append((int(a[0]) - 1, int(a[1]) - 1))             # cv::Point(double, double) truncates

    bias = _structs(_get(mdl, "bias", "model"), "model.bias")
    for b in range(len(bias)):
        path = f"model.bias({b + 1})"
        m.biasw.append(float(np.float32(_scalar(_get(bias[b], "w", path), path + ".w"))))
    m.validate()
    return m


def _row(vals) -> np.ndarray:
    return np.asarray(vals, np.float64).reshape(1, -1) if len(vals) else np.zeros((0, 0))


def serialize(model: Model, filename: str, compress: bool = True) -> bool:
    """The model in the Matlab training code's layout, as a level 5 MAT-file (``save -v7`` when `compress`, ``-v6``
    otherwise).  A child's ``biasid`` of L x K entries (L parent mixtures, K own) is written as the L x K matrix the
    training code builds; every other index array as a row."""
    model.validate()
    filters = MatStruct([{"w": np.asarray(f, np.float64).reshape(f.shape[0], f.shape[1] // model.flen, model.flen)}
                         for f in model.filtersw], ["w"])
    defs = MatStruct([{"w": _row(w), "anchor": _row([a[0] + 1, a[1] + 1, 0])} for w, a in zip(model.defw, model.anchors)],
                     ["w", "anchor"])
    bias = MatStruct([{"w": np.float64(b)} for b in model.biasw], ["w"])
    components = []
    for c in range(model.ncomponents()):
        parts = []
        for p in range(model.nparts(c)):
            par = model.parentid[c][p]
            bid = np.asarray(model.biasid[c][p], np.float64) + 1
            L, K = (len(model.filterid[c][par]), len(model.filterid[c][p])) if par >= 0 else (1, bid.size)
            bid = bid.reshape(L, K) if L > 1 and bid.size == L * K else _row(bid)
            parts.append({"biasid": bid, "filterid": _row(np.asarray(model.filterid[c][p]) + 1),
                          "defid": _row(np.asarray(model.defid[c][p]) + 1), "parent": np.float64(par + 1)})
        components.append(MatStruct(parts, ["biasid", "filterid", "defid", "parent"]))
    mdl = {"filters": filters, "defs": defs, "bias": bias, "components": MatCell(components),
           "interval": np.float64(model.interval), "sbin": np.float64(model.sbin), "thresh": np.float64(model.thresh)}
    matio.savemat(filename, {"name": model.name, "model": mdl}, compress=compress)
    return True
