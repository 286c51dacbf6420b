"""Writes tests/golden/resize_spec_cases.json: what Pillow gives for the preprocessing real checkpoints ask for.

    python tests/golden/make_resize_spec_golden.py

Needs Pillow; recorded with Pillow 12.2.0.  For every spec of tests/resize_spec_reference.SPECS and every case of its
case_list() the file holds
  * the seed, the kind and the shape of the image, and (new_h, new_w, top, left) under the spec;
  * window_sha256: of the 224 x 224 x 3 uint8 window `Image.resize((new_w, new_h), resample)[top:top+224, left:left+224]`.
Hashes, not pixels: the inputs are regenerated from the seeds.  The file holds data only.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from resize_spec_reference import SPECS, case_image, case_list, spec_geometry  # noqa: E402


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    import dataclasses

    import PIL
    from PIL import Image

    cases = [{"name": name, "kind": kind, "seed": seed, "h": h, "w": w} for name, kind, h, w, seed in case_list()]
    specs = {}
    for key, spec in SPECS.items():
        rows = {}
        for name, kind, h, w, seed in case_list():
            new_h, new_w, top, left = spec_geometry(spec, h, w)
            pil = Image.fromarray(case_image(name, kind, h, w, seed))
            window = np.asarray(pil.resize((new_w, new_h), Image.Resampling(spec.resample)))[top : top + 224, left : left + 224]
            rows[name] = {"geometry": [new_h, new_w, top, left], "window_sha256": sha(window)}
        specs[key] = {"spec": dataclasses.asdict(spec), "windows": rows}
        print(key, len(rows), flush=True)
    out = {"pillow": PIL.__version__, "cases": cases, "specs": specs}
    with open(os.path.join(HERE, "resize_spec_cases.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
