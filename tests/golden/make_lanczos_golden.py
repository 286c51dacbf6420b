"""Writes lanczos_cases.json: per case the seed, the shapes and the sha256 of Pillow's `Image.resize(..., Image.LANCZOS)`
output bytes for the seeded "noise" and "binary" images of tests/lanczos_reference.make_image.

    python tests/golden/make_lanczos_golden.py

The file holds data only.  tests/test_lanczos_cpu.py and tests/test_gpu_lanczos.py regenerate the inputs from the seed."""
import hashlib
import json
import os
import sys

import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lanczos_reference import capped_size, make_image  # noqa: E402

# (name, h, w, new_h, new_w); None sizes come from the cap rule of embedder.py:110-114
CASES = [
    # cap-shaped
    ("cap_6x9000", 6, 9000, None, None),
    ("cap_9000x10", 9000, 10, None, None),
    ("cap_8311x12_long_7999", 8311, 12, None, None),
    ("cap_300x8001", 300, 8001, None, None),
    ("cap_4x32768", 4, 32768, 1, 8000),
    # general
    ("gen_37x53", 37, 53, 11, 29),
    ("gen_h_unfiltered", 64, 64, 64, 31),
    ("gen_w_unfiltered", 64, 64, 31, 64),
    ("gen_ratio_15_4_ksize_95", 5, 200, 5, 13),
    ("gen_16x16_to_1x1", 16, 16, 1, 1),
    ("gen_upscale", 7, 9, 20, 23),
    ("gen_1x9000", 1, 9000, 1, 8000),
    ("gen_3x20000", 3, 20000, 1, 8000),
    # tile boundaries of the kernels: 128 output columns and 32 source rows per workgroup of the horizontal pass (4 rows per
    # item), 16 output rows, 1024 row bytes (341 pixels = 1023 bytes, 342 = 1026) and 16-row chunks of the vertical pass
    ("tile_below", 31, 150, 15, 127),
    ("tile_at", 32, 150, 16, 128),
    ("tile_above", 33, 150, 17, 129),
    ("tile_cb_below_chunk_below", 15, 400, 5, 341),
    ("tile_cb_above_chunk_at", 16, 400, 5, 342),
    ("tile_cb_above_chunk_above", 17, 400, 5, 343),
    ("tile_two_bands_two_column_tiles", 70, 700, 33, 683),
    # the 8000 x 8000 output limit, as slivers
    ("limit_sliver_wide", 5, 8100, 4, 8000),
    ("limit_sliver_high", 8100, 5, 8000, 4),
]


def main():
    out = {"pillow": PIL.__version__, "cases": []}
    for seed, (name, h, w, nh, nw) in enumerate(CASES, start=1000):
        if nh is None:
            nh, nw = capped_size(h, w)
        rec = {"name": name, "seed": seed, "h": h, "w": w, "new_h": nh, "new_w": nw, "sha256": {}}
        for kind in ("noise", "binary"):
            img = make_image(seed, h, w, kind)
            res = Image.fromarray(img).resize((nw, nh), Image.LANCZOS)
            assert res.size == (nw, nh)
            rec["sha256"][kind] = hashlib.sha256(res.tobytes()).hexdigest()
        out["cases"].append(rec)
    with open(os.path.join(HERE, "lanczos_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
