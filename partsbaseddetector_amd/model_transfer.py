"""Convert a model file between the Matlab and the FileStorage formats, in either direction:

    python -m partsbaseddetector_amd.model_transfer IN OUT

IN and OUT are ``.mat``, ``.xml``, ``.yml`` or ``.yaml``; the extension chooses the format.  The reference's ModelTransfer
tool (src/ModelTransfer.cpp) only went from ``.mat`` to ``.xml``."""
from __future__ import annotations

import argparse
import sys

from .modelfile import load_model_file, save_model_file


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m partsbaseddetector_amd.model_transfer", description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="model file to read (.mat, .xml, .yml, .yaml)")
    ap.add_argument("output", help="model file to write (.mat, .xml, .yml, .yaml)")
    args = ap.parse_args(argv)
    try:
        model = load_model_file(args.input)
        save_model_file(model, args.output)
    except (OSError, ValueError) as e:
        print(f"model_transfer: {e}", file=sys.stderr)
        return 1
    print(f"{args.input} -> {args.output}: {model.ncomponents()} components, {model.nfilters()} filters")
    return 0


if __name__ == "__main__":
    sys.exit(main())
