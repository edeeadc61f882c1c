"""MAT-file level 5 reader and writer, numpy and zlib only.

The format is MathWorks' published "MAT-File Format" (level 5): a 128-byte header, then one data element per
variable.  Supported subset ("Matlab model files"):

- both byte orders (header endian indicator ``IM`` / ``MI``);
- ``miCOMPRESSED`` elements (one zlib stream holding one element: Matlab's default ``save -v7``), the small data
  element format, 8-byte padding;
- ``miMATRIX`` of the classes double, single, int8..64, uint8..64, char, cell and struct, with the logical flag;
  real data stored in a narrower type than its class (converted to the class); column-major N-d arrays; char data as
  ``miUINT16`` / ``miUTF8`` (and the other character encodings Matlab may write); empty arrays, including a zero-byte
  ``miMATRIX``.

Refused with ValueError: v7.3 files (HDF5), level 4 files, and the classes sparse, object, function handle and opaque,
and complex data.

Values come back as plain Python objects: numeric and logical arrays as numpy arrays indexed as in Matlab (``a[i, j]`` is
``a(i+1, j+1)``), char row vectors as ``str``, cells as ``MatCell`` (a list in Matlab's linear order, plus ``shape``) and
struct arrays as ``MatStruct``.
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Sequence

import numpy as np

# data types (MAT-File Format, table 1-1)
miINT8, miUINT8, miINT16, miUINT16, miINT32, miUINT32, miSINGLE, miDOUBLE = 1, 2, 3, 4, 5, 6, 7, 9
miINT64, miUINT64, miMATRIX, miCOMPRESSED, miUTF8, miUTF16, miUTF32 = 12, 13, 14, 15, 16, 17, 18
_MI_DTYPE = {miINT8: "i1", miUINT8: "u1", miINT16: "i2", miUINT16: "u2", miINT32: "i4", miUINT32: "u4",
             miSINGLE: "f4", miDOUBLE: "f8", miINT64: "i8", miUINT64: "u8"}

# array classes (table 1-3)
mxCELL, mxSTRUCT, mxOBJECT, mxCHAR, mxSPARSE, mxDOUBLE, mxSINGLE = 1, 2, 3, 4, 5, 6, 7
mxINT8, mxUINT8, mxINT16, mxUINT16, mxINT32, mxUINT32, mxINT64, mxUINT64, mxFUNCTION, mxOPAQUE = range(8, 18)
_MX_DTYPE = {mxDOUBLE: "f8", mxSINGLE: "f4", mxINT8: "i1", mxUINT8: "u1", mxINT16: "i2", mxUINT16: "u2",
             mxINT32: "i4", mxUINT32: "u4", mxINT64: "i8", mxUINT64: "u8"}
_MX_NAME = {mxCELL: "cell", mxSTRUCT: "struct", mxOBJECT: "object", mxCHAR: "char", mxSPARSE: "sparse", mxDOUBLE: "double",
            mxSINGLE: "single", mxINT8: "int8", mxUINT8: "uint8", mxINT16: "int16", mxUINT16: "uint16", mxINT32: "int32",
            mxUINT32: "uint32", mxINT64: "int64", mxUINT64: "uint64", mxFUNCTION: "function handle", mxOPAQUE: "opaque"}
_FLAG_COMPLEX, _FLAG_LOGICAL = 0x0800, 0x0200
_HDF5_SIGNATURE = b"\x89HDF\r\n\x1a\n"
_RESAVE = "re-save it in Matlab with save -v7"


class MatCell(list):
    """A Matlab cell array: its elements in Matlab's linear (column-major) order, and its ``shape``."""

    def __init__(self, items: Sequence = (), shape=None):
        super().__init__(items)
        self.shape = tuple(shape) if shape is not None else (1, len(self))
        if int(np.prod(self.shape)) != len(self):
            raise ValueError(f"cell of shape {self.shape} cannot hold {len(self)} elements")

    def __repr__(self):
        return f"MatCell({list.__repr__(self)}, shape={self.shape})"


class MatStruct:
    """A Matlab struct array: ``shape``, ``fieldnames`` (file order) and ``elements`` (one dict per element, Matlab's
    linear order).  ``s[k]`` is element k's dict; ``len(s)`` the number of elements."""

    def __init__(self, elements: Sequence[Dict], fieldnames: Sequence[str] = None, shape=None):
        self.elements: List[Dict] = [dict(e) for e in elements]
        if fieldnames is None:
            fieldnames = list(self.elements[0]) if self.elements else []
        self.fieldnames: List[str] = list(fieldnames)
        self.shape = tuple(shape) if shape is not None else (1, len(self.elements))
        if int(np.prod(self.shape)) != len(self.elements):
            raise ValueError(f"struct of shape {self.shape} cannot hold {len(self.elements)} elements")
        for e in self.elements:
            if set(e) != set(self.fieldnames):
                raise ValueError(f"struct element fields {sorted(e)} differ from {sorted(self.fieldnames)}")

    def __len__(self):
        return len(self.elements)

    def __getitem__(self, k) -> Dict:
        return self.elements[k]

    def __iter__(self):
        return iter(self.elements)

    def __repr__(self):
        return f"MatStruct(shape={self.shape}, fieldnames={self.fieldnames})"


# ------------------------------------------------------------------------------------------ reader
def _tag(buf, pos: int, end: int, bo: str, where: str):
    """one data element at buf[pos:end]: (type, payload, position of the next element)"""
    if pos + 8 > end:
        raise ValueError(f"{where}: truncated data element")
    first, = struct.unpack_from(bo + "I", buf, pos)
    if first >> 16:                                           # small data element: type and size in one word
        mtype, n = first & 0xFFFF, first >> 16
        if n > 4:
            raise ValueError(f"{where}: small data element of {n} bytes")
        return mtype, bytes(buf[pos + 4:pos + 4 + n]), pos + 8
    mtype = first
    n, = struct.unpack_from(bo + "I", buf, pos + 4)
    start = pos + 8
    if n > end - start:
        raise ValueError(f"{where}: data element of {n} bytes runs past the end of its container")
    nxt = start + n if mtype == miCOMPRESSED else start + ((n + 7) & ~7)
    return mtype, bytes(buf[start:start + n]), min(nxt, end)


def _numbers(mtype: int, data: bytes, bo: str, where: str) -> np.ndarray:
    if mtype not in _MI_DTYPE:
        raise ValueError(f"{where}: data type {mtype} is not numeric")
    dt = np.dtype(bo + _MI_DTYPE[mtype])
    if len(data) % dt.itemsize:
        raise ValueError(f"{where}: {len(data)} bytes is not a whole number of {dt.name} values")
    return np.frombuffer(data, dt).astype(dt.newbyteorder("="))


def _chars(mtype: int, data: bytes, bo: str, where: str) -> str:
    if mtype == miUTF8:
        return data.decode("utf-8")
    if mtype == miUTF16:
        return data.decode("utf-16-le" if bo == "<" else "utf-16-be")
    if mtype in (miUINT8, miINT8):
        return data.decode("latin-1")
    if mtype in (miUINT16, miINT16, miUTF32, miUINT32, miINT32):
        codes = _numbers({miUTF32: miUINT32}.get(mtype, mtype), data, bo, where)
        return "".join(map(chr, codes.astype(np.int64)))
    raise ValueError(f"{where}: character data of type {mtype}")


def _matrix(data: bytes, bo: str, where: str, depth: int = 0):
    """the value of one miMATRIX element's payload; `where` names it in errors (variable name or path)"""
    if depth > 64:
        raise ValueError(f"{where}: nested more than 64 levels deep")
    if len(data) == 0:                                        # what Matlab writes for some empty cells and fields
        return np.zeros((0, 0))
    end = len(data)
    t, flags, pos = _tag(data, 0, end, bo, where)
    if t != miUINT32 or len(flags) != 8:
        raise ValueError(f"{where}: bad array flags")
    word = _numbers(miUINT32, flags, bo, where)[0]
    cls = int(word & 0xFF)
    t, dims, pos = _tag(data, pos, end, bo, where)
    dims = tuple(int(d) for d in _numbers(t, dims, bo, where)) if t == miINT32 else None
    if dims is None or len(dims) < 2 or min(dims) < 0:
        raise ValueError(f"{where}: bad dimensions")
    t, name, pos = _tag(data, pos, end, bo, where)
    if t != miINT8:
        raise ValueError(f"{where}: bad array name")
    if not where:
        where = name.decode("latin-1")
    if cls not in _MX_DTYPE and cls not in (mxCHAR, mxCELL, mxSTRUCT):
        raise ValueError(f"variable {where!r}: Matlab class {_MX_NAME.get(cls, cls)!r} is not supported")
    if word & _FLAG_COMPLEX:
        raise ValueError(f"variable {where!r}: complex {_MX_NAME[cls]} data is not supported")
    count = int(np.prod([float(d) for d in dims]))
    if count > 8 * len(data):
        raise ValueError(f"{where}: dimensions {dims} larger than the data")

    if cls in _MX_DTYPE:
        t, real, pos = _tag(data, pos, end, bo, where)
        a = _numbers(t, real, bo, where)
        if a.size != count:
            raise ValueError(f"{where}: {a.size} values for dimensions {dims}")
        a = a.astype(bool) if word & _FLAG_LOGICAL else a.astype(_MX_DTYPE[cls])
        return a.reshape(dims, order="F")
    if cls == mxCHAR:
        text = ""
        if pos < end:
            t, raw, pos = _tag(data, pos, end, bo, where)
            text = _chars(t, raw, bo, where)
        if len(text) != count:
            raise ValueError(f"{where}: {len(text)} characters for dimensions {dims}")
        if len(dims) == 2 and dims[0] <= 1:
            return text
        return np.array(list(text), dtype="<U1").reshape(dims, order="F")
    if cls == mxCELL:
        items = []
        for k in range(count):
            sub = f"{where}{{{k + 1}}}"
            t, raw, pos = _tag(data, pos, end, bo, sub)
            if t != miMATRIX:
                raise ValueError(f"{sub}: cell element is not an array")
            items.append(_matrix(raw, bo, sub, depth + 1))
        return MatCell(items, dims)
    # mxSTRUCT
    t, raw, pos = _tag(data, pos, end, bo, where)
    fl = _numbers(t, raw, bo, where) if t == miINT32 else []
    if len(fl) != 1 or fl[0] <= 0:
        raise ValueError(f"{where}: bad struct field name length")
    fl = int(fl[0])
    t, raw, pos = _tag(data, pos, end, bo, where)
    if t != miINT8 or len(raw) % fl:
        raise ValueError(f"{where}: bad struct field names")
    names = [raw[i:i + fl].split(b"\0", 1)[0].decode("latin-1") for i in range(0, len(raw), fl)]
    elements = []
    for k in range(count):
        el = {}
        for f in names:
            sub = f"{where}({k + 1}).{f}" if count != 1 else f"{where}.{f}"
            t, raw, pos = _tag(data, pos, end, bo, sub)
            if t != miMATRIX:
                raise ValueError(f"{sub}: struct field is not an array")
            el[f] = _matrix(raw, bo, sub, depth + 1)
        elements.append(el)
    return MatStruct(elements, names, dims)


def _header_byteorder(buf: bytes, filename: str) -> str:
    if len(buf) < 4 or 0 in buf[:4]:
        raise ValueError(f"{filename}: not a MAT-file level 5 (a level 4 file, or not a MAT-file at all); {_RESAVE}")
    if len(buf) < 128:
        raise ValueError(f"{filename}: truncated MAT-file header")
    if b"MATLAB 7.3" in buf[:116] or buf[512:520] == _HDF5_SIGNATURE:
        raise ValueError(f"{filename}: a v7.3 MAT-file is HDF5, which this reader does not read; {_RESAVE}")
    ind = buf[126:128]
    if ind not in (b"IM", b"MI"):
        raise ValueError(f"{filename}: not a MAT-file level 5 (no endian indicator); {_RESAVE}")
    bo = "<" if ind == b"IM" else ">"
    version, = struct.unpack_from(bo + "H", buf, 124)
    if version != 0x0100:
        raise ValueError(f"{filename}: MAT-file version 0x{version:04x} is not level 5; {_RESAVE}")
    return bo


def loadmat(filename: str) -> Dict[str, object]:
    """Every variable of a level 5 MAT-file, by name, in file order."""
    with open(filename, "rb") as fh:
        buf = fh.read()
    bo = _header_byteorder(buf, filename)
    out: Dict[str, object] = {}
    pos = 128
    while pos < len(buf):
        if len(buf) - pos < 8 and not any(buf[pos:]):
            break                                             # trailing padding
        t, raw, pos = _tag(buf, pos, len(buf), bo, filename)
        if t == miCOMPRESSED:
            try:
                raw = zlib.decompress(raw)
            except zlib.error as e:
                raise ValueError(f"{filename}: corrupt compressed element ({e})") from None
            t, raw, _ = _tag(raw, 0, len(raw), bo, filename)
        if t != miMATRIX:
            raise ValueError(f"{filename}: top-level data element of type {t} is not an array")
        name = _peek_name(raw, bo, filename)
        out[name] = _matrix(raw, bo, name)
    return out


def _peek_name(raw: bytes, bo: str, where: str) -> str:
    if not raw:
        raise ValueError(f"{where}: a top-level variable without a header")
    _, _, pos = _tag(raw, 0, len(raw), bo, where)
    _, _, pos = _tag(raw, pos, len(raw), bo, where)
    t, name, _ = _tag(raw, pos, len(raw), bo, where)
    if t != miINT8 or not name:
        raise ValueError(f"{where}: a top-level variable without a name")
    return name.decode("latin-1")


# ------------------------------------------------------------------------------------------ writer
def _element(mtype: int, payload: bytes) -> bytes:
    n = len(payload)
    if 0 < n <= 4 and mtype != miMATRIX:                      # small data element format
        return struct.pack("<HH", mtype, n) + payload.ljust(4, b"\0")
    return struct.pack("<II", mtype, n) + payload + b"\0" * (-n % 8)


def _array(cls: int, dims, name: str, body: bytes, logical: bool = False) -> bytes:
    flags = struct.pack("<II", cls | (_FLAG_LOGICAL if logical else 0), 0)
    head = (_element(miUINT32, flags) + _element(miINT32, np.asarray(dims, "<i4").tobytes())
            + _element(miINT8, name.encode("latin-1")))
    return _element(miMATRIX, head + body)


_DTYPE_MX = {v: k for k, v in _MX_DTYPE.items()}
_DTYPE_MI = {v: k for k, v in _MI_DTYPE.items()}


def _value(v, name: str = "") -> bytes:
    if isinstance(v, str):
        dims = (1, len(v)) if v else (0, 0)
        codes = np.array([ord(c) for c in v], "<u2")
        return _array(mxCHAR, dims, name, _element(miUINT16, codes.tobytes()))
    if isinstance(v, MatStruct) or isinstance(v, dict):
        s = v if isinstance(v, MatStruct) else MatStruct([v])
        fl = max([len(f) for f in s.fieldnames] + [0]) + 1
        body = _element(miINT32, struct.pack("<i", fl))
        body += _element(miINT8, b"".join(f.encode("latin-1").ljust(fl, b"\0") for f in s.fieldnames))
        for el in s.elements:
            for f in s.fieldnames:
                body += _value(el[f])
        return _array(mxSTRUCT, s.shape, name, body)
    if isinstance(v, (list, tuple)):
        c = v if isinstance(v, MatCell) else MatCell(v)
        return _array(mxCELL, c.shape, name, b"".join(_value(x) for x in c))
    a = np.asarray(v, np.float64) if isinstance(v, (bool, int, float)) else np.asarray(v)   # a Matlab literal is a double
    if a.ndim < 2:
        a = a.reshape(1, -1) if a.size or a.ndim == 1 else a.reshape(0, 0)
    logical = a.dtype == np.bool_
    if logical:
        a = a.astype(np.uint8)
    code = a.dtype.newbyteorder("=").str.lstrip("<>=|")
    if code not in _DTYPE_MX:
        raise ValueError(f"variable {name!r}: numpy type {a.dtype} has no Matlab class")
    data = np.asarray(a, a.dtype.newbyteorder("<")).ravel(order="F").tobytes()
    return _array(_DTYPE_MX[code], a.shape, name, _element(_DTYPE_MI[code], data), logical)


def savemat(filename: str, variables: Dict[str, object], compress: bool = True) -> None:
    """Write `variables` as a little-endian level 5 MAT-file (each variable in its own miCOMPRESSED element when
    `compress`, as Matlab's ``save -v7``; plain elements as ``save -v6`` otherwise).  Values: str (char row), numpy arrays
    and Python numbers (numeric; bool arrays as logical; 0-d and 1-d arrays become row vectors), MatCell / list (cell),
    MatStruct / dict (struct)."""
    text = b"MATLAB 5.0 MAT-file, written by partsbaseddetector_amd.matio"
    out = [text.ljust(116, b" ") + b"\0" * 8 + struct.pack("<H", 0x0100) + b"IM"]
    for name, v in variables.items():
        el = _value(v, name)
        if compress:
            z = zlib.compress(el)
            el = struct.pack("<II", miCOMPRESSED, len(z)) + z
        out.append(el)
    with open(filename, "wb") as fh:
        fh.write(b"".join(out))
