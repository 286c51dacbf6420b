#!/usr/bin/env python3
"""The encoder family side by side: ViT-S/16, ViT-B/16 and ViT-L/16 on the same crops in one process.

    python tools/bench_vit_family.py [--crops 4096] [--chunk 4096] [--steps 5] [--warmup 2] [--out profiles/vit_family.json]

For each geometry: seeded weights (weights.make_vit_weights), one context, `--crops` synthetic 224 x 224 crops resident
on the device, `--warmup` untimed and `--steps` timed calls of mme_embed (K1 + the whole forward; bench.py's defaults),
timed by one pair of HIP events around the timed calls.  ViT-B/16 is measured twice, first and last: the difference of
its two figures is the noise floor of the run, the margin of every comparison made from this table.

Per geometry: ms_per_step, crops/s, FLOP per crop (weights.vit_flops_per_crop), the achieved FLOP/s of the whole call
as a fraction of the nominal 2.5 PFLOP/s dense bf16 peak (an end-to-end figure: it includes the preprocessing and the
row kernels, it is not a kernel's share of peak) and the attention layers of the last pass that were redone exactly.
Prints a table and ONE JSON line, which it also writes to --out (DESIGN.md 4.6 quotes it).  Needs a GPU; no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NOMINAL_FLOPS = 2.5e15  # dense bf16 MFMA peak of the MI355X, as bench.py prices its headline


def measure(name, geom, pix, offs, hw, args):
    import torch

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import make_vit_weights, vit_flops_per_crop

    t0 = time.perf_counter()
    w = make_vit_weights(1, geom)
    eng = Engine(0)
    eng.load_vit(w, geom=geom)
    del w
    eng.set_chunk(args.chunk)
    n, d = len(offs), eng.embed_dim
    e32 = torch.empty((n, d), dtype=torch.float32, device=pix.device)
    e16 = torch.empty((n, d), dtype=torch.bfloat16, device=pix.device)
    for _ in range(args.warmup):
        eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.steps):
        eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / args.steps
    redone = eng.attention_redone(geom.num_layers)
    if not bool(torch.isfinite(e32).all()):
        raise SystemExit(f"{name}: non-finite embeddings")
    eng.close()
    flop = vit_flops_per_crop(geom)
    rate = n / (ms * 1e-3)
    row = {"name": name, "hidden": geom.hidden_size, "layers": geom.num_layers, "heads": geom.num_heads, "mlp": geom.intermediate_size,
           "ms_per_step": ms, "crops_per_s": rate, "flop_per_crop": flop, "frac_of_nominal": flop * rate / NOMINAL_FLOPS,
           "attention_layers_redone": int(sum(1 for f in redone if f)), "setup_s": setup_s}
    print(f"{name:12s} {geom.hidden_size:5d} x {geom.num_layers:2d}  {ms:9.2f} ms/step  {rate:10.0f} crops/s  {flop / 1e9:8.2f} GFLOP/crop  "
          f"{row['frac_of_nominal']:.4f} of nominal  redone {row['attention_layers_redone']}", flush=True)
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--crops", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_family.json"))
    args = ap.parse_args(argv)
    if args.crops < 1 or args.steps < 1 or args.warmup < 0:
        ap.error("--crops and --steps must be positive, --warmup non-negative")

    import numpy as np
    import torch

    from multimodal_embeddings_amd.build import kernel_source_hash
    from multimodal_embeddings_amd.weights import VIT_B16, VIT_L16, VIT_S16, synthetic_crops

    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_family: no GPU visible; this is a GPU measurement and has no fallback")
    dev = torch.device("cuda:0")
    n = args.crops
    pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
    for b0 in range(0, n, 4096):
        blk = synthetic_crops(min(4096, n - b0), seed=0, start=b0)
        pix[b0 * 150528 : (b0 + len(blk)) * 150528] = torch.from_numpy(blk.reshape(-1)).to(dev)
    offs = np.arange(n, dtype=np.int64) * 150528
    hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
    order = [("vit_b16_first", VIT_B16), ("vit_s16", VIT_S16), ("vit_l16", VIT_L16), ("vit_b16_last", VIT_B16)]
    rows = [measure(name, geom, pix, offs, hw, args) for name, geom in order]
    by = {r["name"]: r for r in rows}
    margin = abs(by["vit_b16_first"]["frac_of_nominal"] - by["vit_b16_last"]["frac_of_nominal"])
    b_best = max(by["vit_b16_first"]["frac_of_nominal"], by["vit_b16_last"]["frac_of_nominal"])
    b_low = min(by["vit_b16_first"]["frac_of_nominal"], by["vit_b16_last"]["frac_of_nominal"])
    result = {"tool": "bench_vit_family", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "crops": n,
              "chunk": args.chunk, "steps": args.steps, "warmup": args.warmup, "nominal_flops": NOMINAL_FLOPS, "rows": rows,
              "vit_b16_margin_frac": margin,
              # the expectation DESIGN.md 4.6 states: ViT-L's fraction is no lower than ViT-B's, to within the run's own noise
              "vit_l16_frac_minus_vit_b16_low": by["vit_l16"]["frac_of_nominal"] - b_low,
              "vit_l16_not_below_vit_b16": bool(by["vit_l16"]["frac_of_nominal"] >= b_best - margin)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
