"""Writes tests/golden/clip_preprocess_cases.json: what Pillow and transformers give for CLIP's own preprocessing.

    python tests/golden/make_clip_preprocess_golden.py

Needs Pillow and transformers (CLIPImageProcessorPil); recorded with Pillow 12.2.0 and transformers 5.15.0.  For every
case of tests/clip_preprocess_reference.case_list() and every bundled crop of tests/golden/crops/ the file holds
  * the seed or the crop's file name, the shape and (new_h, new_w, top, left);
  * window_sha256: of the 224 x 224 x 3 uint8 window `Image.resize((new_w, new_h), BICUBIC)[top:top+224, left:left+224]`;
  * pixel_values_sha256: of the f32 [3, 224, 224] array CLIPImageProcessorPil returned.
Hashes, not pixels: the inputs are regenerated from the seeds or read from the bundled crops.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from clip_preprocess_reference import case_image, case_list, clip_resize_geometry  # noqa: E402


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    import PIL
    import transformers
    from PIL import Image
    from transformers import CLIPImageProcessorPil

    proc = CLIPImageProcessorPil()  # CLIP's defaults: shortest_edge 224, BICUBIC, centre crop 224, CLIP mean / std

    def record(img: np.ndarray) -> dict:
        h, w = img.shape[:2]
        new_h, new_w, top, left = clip_resize_geometry(h, w)
        pil = Image.fromarray(img)
        window = np.asarray(pil.resize((new_w, new_h), Image.BICUBIC))[top : top + 224, left : left + 224]
        pv = np.asarray(proc(images=[pil], return_tensors="np")["pixel_values"][0], dtype=np.float32)
        assert pv.shape == (3, 224, 224)
        return {"h": h, "w": w, "geometry": [new_h, new_w, top, left], "window_sha256": sha(window), "pixel_values_sha256": sha(pv)}

    cases = []
    for name, kind, h, w, seed in case_list():
        cases.append({"name": name, "kind": kind, "seed": seed, **record(case_image(kind, h, w, seed))})
        print(name, cases[-1]["geometry"], flush=True)
    for name in sorted(f for f in os.listdir(os.path.join(HERE, "crops")) if f.endswith(".png")):
        img = np.asarray(Image.open(os.path.join(HERE, "crops", name)).convert("RGB"))
        cases.append({"name": name, "kind": "bundled", "seed": None, **record(img)})
    out = {"pillow": PIL.__version__, "transformers": transformers.__version__, "cases": cases}
    with open(os.path.join(HERE, "clip_preprocess_cases.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"{len(cases)} cases")


if __name__ == "__main__":
    main()
