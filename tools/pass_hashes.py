#!/usr/bin/env python3
"""sha256 of what every encoder pass writes, per configuration: one JSON line each.

    python tools/pass_hashes.py [--only image|text|tile] > hashes.jsonl

For a change that moves no arithmetic (the transformer block's launch sequence is host code: csrc/encoder_pass.hip) the
lines of two libraries must be EQUAL, not close.  Run the tool once per library, each in a fresh process -- another
build is selected with MME_LIB_PATH and MME_ALLOW_LIB_OVERRIDE=1, as tools/_diag.py does -- and compare the outputs with
`diff`.  Every tower is two layers deep and seeded (weights.py), every input is seeded; the shapes are the smallest that
reach every branch of the shared block:

  image   ViT-S/16 width (384: no partial planes under ln_mode 2), ViT-B/16 width (768: planes), CLIP-B/16 (pre-LN,
          QuickGELU, projection), ViT-B/32, CLIP-B/32.  3 crops at patch 16 are 591 rows (two 256-row panels and a ragged
          tail of 79), 6 crops at patch 32 are 300.  From the defaults one switch at a time: ln_mode, tile order, attention
          mode, last-layer pruning at the first and the last pool token, GEMM variant, and chunks of 2 over 5 crops.
  text    CLIP-B's text width with and without projection, 3 sequences; once more than one chunk of 1024.
  tile    1 local + 1 global layer, one intermediate state, both save-point conventions, ln_mode 1 / 2 x attention mode
          0 / 1 / 2, on a 1-tile and a 4-tile image.

Each configuration ends in a device synchronise; the first error ends the run (nothing is caught).  Needs a GPU.
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("image", "text", "tile"), default=None)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from multimodal_embeddings_amd import weights as W
    from multimodal_embeddings_amd._lib import Engine

    if not torch.cuda.is_available():
        raise SystemExit("pass_hashes: no GPU visible; the passes run on the GPU and there is no fallback")

    def pack(arrays):
        """list of uint8 [h, w, 3] -> (pix CUDA tensor, offs int64 [n], hw int32 [n, 2]), every crop 16-byte aligned"""
        hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
        sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
        offs = np.zeros(len(arrays), dtype=np.int64)
        offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
        buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
        for a, o, n in zip(arrays, offs, sizes):
            buf[o : o + n] = a.reshape(-1)
        return torch.from_numpy(buf).to("cuda:0"), offs, hw

    def emit(config: str, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        print(json.dumps({"config": config, "sha256": h.hexdigest()}), flush=True)

    def image():
        two = {"num_layers": 2}
        towers = {
            "vit_s16": dataclasses.replace(W.VIT_S16, **two), "vit_b16": dataclasses.replace(W.VIT_B16, **two),
            "clip_b16": dataclasses.replace(W.CLIP_B16, **two), "vit_b32": dataclasses.replace(W.VIT_B32, **two),
            "clip_b32": dataclasses.replace(W.CLIP_B32, **two),
        }
        # (name, setter, values): the first value is the library's default and is restored after the sweep
        switches = [("ln_mode", Engine.set_ln_fusion, (2, 0, 1)), ("tile_order", Engine.set_tile_order, (1, 0, 2)),
                    ("attention_mode", Engine.set_attention_mode, (1, 0, 2)), ("gemm_variant", Engine.set_gemm_variant, (0, 1, 3))]
        for name, geom in towers.items():
            clip = isinstance(geom, W.CLIPGeometry)
            e = Engine(0)
            (e.load_clip if clip else e.load_vit)((W.make_clip_weights if clip else W.make_vit_weights)(11, geom), geom=geom)
            n = 3 if geom.patch_size == 16 else 6
            patches = e.preprocess(*pack(list(W.synthetic_crops(n, seed=5))))
            emit(f"{name} defaults", *e.vit_forward(patches))
            for sw, setter, values in switches:
                for v in values[1:]:
                    setter(e, v)
                    emit(f"{name} {sw}={v}", *e.vit_forward(patches))
                setter(e, values[0])
            e.set_forward_pruning(True)
            for tok in (0, geom.seq_len - 1):
                emit(f"{name} pruned pool_token={tok}", *e.vit_forward(patches, pool_token=tok))
            e.set_forward_pruning(False)
            e.set_chunk(2)
            emit(f"{name} chunk=2 n=5", *e.vit_forward(e.preprocess(*pack(list(W.synthetic_crops(5, seed=6))))))
            e.close()

    def text():
        for proj in (512, None):
            geom = W.CLIPTextGeometry(num_layers=2, vocab_size=256, eos_token_id=255, projection_dim=proj)
            e = Engine(0)
            e.load_clip_text(W.make_clip_text_weights(41, geom), geom)
            for n in (3, 1030) if proj else (3,):  # MME_TEXT_CHUNK is 1024: a full chunk and a ragged one
                emit(f"text projection={proj} n={n}", *e.text_forward(W.synthetic_token_ids(n, geom.vocab_size, geom.eos_token_id, 7)))
            e.close()

    def tile():
        rng = np.random.default_rng(4)
        arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(300, 200, 3), (1000, 1100, 3)]]
        w = None
        for point in ("after", "before"):
            geom = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,), intermediate_save_point=point)
            w = w or W.make_tile_vit_weights(3, geom)  # the tensors do not depend on the save point
            e = Engine(0)
            e.load_tile_vit(w, geom)
            pv, ids, _, nt = e.preprocess_tiles(*pack(arrays), 560, 4)
            assert nt == [1, 4], nt
            for ln in (1, 2):
                e.set_ln_fusion(ln)
                for attn in (0, 1, 2):
                    e.set_attention_mode(attn)
                    emit(f"tile save={point} ln_mode={ln} attention_mode={attn}", *e.tile_vit_forward(pv, ids, nt, want_hidden=True))
            e.close()

    for name, fn in (("image", image), ("text", text), ("tile", tile)):
        if args.only in (None, name):
            fn()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
