"""Model files by extension: the FileStorage documents (``.xml``, ``.yml``, ``.yaml``: filestorage.py) and the Matlab
training code's MAT-files (``.mat``: matlab_model.py), as the reference's demo chooses its reader (src/demo.cpp:63-77)."""
from __future__ import annotations

import os

from . import filestorage, matlab_model
from .model import Model

MODEL_EXTENSIONS = (".xml", ".yml", ".yaml", ".mat")


def _ext(path: str) -> str:
    ext = os.path.splitext(path)[1].lower()
    if ext not in MODEL_EXTENSIONS:
        raise ValueError(f"{path}: unsupported model format {ext or '(no extension)'!r}; expected one of {', '.join(MODEL_EXTENSIONS)}")
    return ext


def load_model_file(path: str) -> Model:
    """The model in `path`, read by the reader its extension names."""
    return matlab_model.deserialize(path) if _ext(path) == ".mat" else filestorage.deserialize(path)


def save_model_file(model: Model, path: str) -> None:
    """`model` written to `path` in the format its extension names (``.mat``: compressed, as Matlab's ``save -v7``)."""
    ext = _ext(path)
    if ext == ".mat":
        matlab_model.serialize(model, path)
    elif ext == ".xml":
        filestorage.serialize_xml(model, path)
    else:
        filestorage.serialize(model, path)
