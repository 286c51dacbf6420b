#!/usr/bin/env python3
"""encoder="mllama" (DESIGN.md 4.30): what the projector and the language tower add to the tile tower, per image.

    python tools/bench_mllama.py [--chunks 1,8,64] [--out profiles/mllama_lm.json]

The tile tower runs at the checkpoint's full depth (32 + 8 layers).  The language tower runs at the checkpoint's WIDTH (4096 / 32 / 8
heads, MLP 14336, vision rows of 7680) in two SHALLOWER stacks with the checkpoint's layer mix -- 5 layers (cross layer 3) and 10
layers (cross layers 3, 8), vocabulary cut to 32000 ids -- because seeding 9.3 G weights on the host takes longer than every
measurement together.  Per figure: t5, t10 measured (median of 7 after 2 warm-up passes, events on the stream), and the full 40
layers (8 blocks of 4 self + 1 cross) as t5 + 7 (t10 - t5), LABELLED "scaled".  What does not scale with depth (the gather, the
projector GEMM, the pooling) is in t5 once, as in the full tower.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_embeddings_amd._lib import Engine
from multimodal_embeddings_amd.embedder import RegionEmbedder
from multimodal_embeddings_amd.weights import MLLAMA_LM_11B, make_mllama_lm_weights, make_tile_vit_weights

PROMPT = [128000 % 32000, 32000, 128000 % 32000, 1101, 1102, 1103, 1104, 1105]  # BOS, <|image|>, BOS, five words: the reference prompt's shape
REPS, WARM = 7, 2


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(float(a.elapsed_time(b)))
    return float(np.median(ms)), ms


def classes(eng, fn):
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile(False)
    return {k: round(v[0], 3) for k, v in prof.items() if v[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="1,8,64")
    ap.add_argument("--out", default=os.path.join("profiles", "mllama_lm.json"))
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    nmax = max(chunks)
    eng = Engine(0)
    t0 = time.time()
    eng.load_tile_vit(make_tile_vit_weights(2))
    print(f"tile tower seeded and loaded in {time.time() - t0:.0f} s", flush=True)
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (1000 + 7 * (k % 8), 1100, 3), dtype=np.uint8) for k in range(nmax)]
    pix, offs, hw = RegionEmbedder(engine=eng).pack(arrays)
    pv, ids, _, nt = eng.preprocess_tiles(pix, offs, hw, 560, 4)
    ids, nt = np.asarray(ids), np.asarray(nt)
    assert int(nt.min()) == 4
    result = {"what": "ms per call, median of 7; language tower at full width, 5- and 10-layer stacks, 40 layers SCALED as t5 + 7 (t10 - t5)",
              "prompt_tokens": len(PROMPT), "tile_tower": {}, "embed": {}, "text_only": {}}
    for c in chunks:
        eng.set_chunk(c)
        med, all_ms = timed(lambda: eng.tile_vit_forward(pv[:c], ids[:c], nt[:c], want_bf16=False))
        result["tile_tower"][str(c)] = {"ms": med, "ms_per_image": med / c, "runs": all_ms}
        print(f"tile tower alone, chunk {c}: {med:.1f} ms = {med / c:.2f} ms per image", flush=True)
    for depth, cross in ((5, (3,)), (10, (3, 8))):
        geom = dataclasses.replace(MLLAMA_LM_11B, num_layers=depth, cross_attention_layers=cross, vocab_size=32000, image_token_id=32000)
        t0 = time.time()
        eng.load_mllama_lm(make_mllama_lm_weights(7, geom), geom)
        print(f"language tower, {depth} layers, seeded and loaded in {time.time() - t0:.0f} s", flush=True)
        for c in chunks:
            eng.set_chunk(c)
            prompt = np.tile(np.asarray(PROMPT, dtype=np.int32), (c, 1))
            call = lambda: eng.mllama_embed(pv[:c], ids[:c], nt[:c], prompt, want_bf16=False)  # noqa: E731
            med, all_ms = timed(call)
            result["embed"].setdefault(str(c), {})[f"t{depth}"] = {"ms": med, "runs": all_ms, "classes_ms": classes(eng, call)}
            print(f"mllama_embed, {depth} layers, chunk {c}: {med:.1f} ms", flush=True)
        for n in (1, 64):
            eng.set_chunk(64)
            text = np.tile(np.arange(1000, 1016, dtype=np.int32), (n, 1))
            call = lambda: eng.mllama_lm_forward(text, want_bf16=False)  # noqa: E731
            med, all_ms = timed(call)
            result["text_only"].setdefault(str(n), {})[f"t{depth}"] = {"ms": med, "runs": all_ms, "classes_ms": classes(eng, call)}
            print(f"text only, {depth} layers, {n} x 16 tokens: {med:.2f} ms", flush=True)
    for c in chunks:
        r = result["embed"][str(c)]
        full = r["t5"]["ms"] + 7 * (r["t10"]["ms"] - r["t5"]["ms"])
        tile = result["tile_tower"][str(c)]["ms"]
        r["scaled_40_layers"] = {"ms": full, "ms_per_image": full / c, "added_ms_per_image": (full - tile) / c, "label": "scaled"}
        print(f"chunk {c}: 40 layers (scaled) {full / c:.2f} ms per image, of which the tile tower {tile / c:.2f}: the language side adds {(full - tile) / c:.2f}")
    for n in ("1", "64"):
        r = result["text_only"][n]
        r["scaled_40_layers"] = {"ms": r["t5"]["ms"] + 7 * (r["t10"]["ms"] - r["t5"]["ms"]), "label": "scaled (32 self layers; the cross layers are skipped)"}
        print(f"text only, {n} x 16 tokens: 40 layers (scaled) {r['scaled_40_layers']['ms']:.2f} ms")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
