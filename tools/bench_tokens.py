#!/usr/bin/env python3
"""Patch-token rows, measured: the token pass beside the plain embed on the same crops in one process.

    python tools/bench_tokens.py [--crops 1024] [--steps 7] [--warmup 3] [--out profiles/tokens.json]

Seeded ViT-B/16 and DINOv2-B/14, `--crops` synthetic crops in one chunk: mme_embed against mme_embed_tokens (the default window,
the patch tokens), with forward pruning off and on.  The difference is the token kernel -- whose algorithmic traffic is one
read of the window's residual rows and one write of the token rows -- plus, under the pruning setting, the last block run in
full.  Every timed call sits between its own pair of HIP events: median and range.  Then one token pass under
mme_profile_enable: kernel time by class.  Prints a table and writes ONE JSON document.  Needs a GPU; no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # as bench.py


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def token_pass(name, args):
    import numpy as np
    import torch

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import DINOV2_B14, VIT_B16, make_dinov2_weights, make_vit_weights, synthetic_crops

    dev = torch.device("cuda:0")
    n = args.crops
    pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
    pix[: n * 150528] = torch.from_numpy(synthetic_crops(n, seed=0).reshape(-1)).to(dev)
    offs = np.arange(n, dtype=np.int64) * 150528
    hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
    eng = Engine(0)
    if name == "dinov2_b14":
        eng.load_dinov2(make_dinov2_weights(1, DINOV2_B14), DINOV2_B14)
    else:
        eng.load_vit(make_vit_weights(1, VIT_B16), geom=VIT_B16)
    eng.set_chunk(n)
    g = eng.vit_geometry()
    ntok, d = g.num_patches, g.hidden_size
    e32 = torch.empty((n, d), dtype=torch.float32, device=dev)
    e16 = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    tok = torch.empty((n, ntok, d), dtype=torch.bfloat16, device=dev)
    row = {"name": name, "crops": n, "ntok": ntok, "hidden": d, "token_bytes": n * ntok * d * 2}
    for prune in (False, True):
        eng.set_forward_pruning(prune)
        tag = "pruned" if prune else "full"
        row[f"embed_{tag}"] = timed(torch, lambda: eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16), args.steps, args.warmup)
        row[f"embed_tokens_{tag}"] = timed(torch, lambda: eng.embed_tokens(pix, offs, hw, 0, out=tok, out_f32=e32, out_bf16=e16), args.steps, args.warmup)
        row[f"extra_ms_{tag}"] = row[f"embed_tokens_{tag}"]["median_ms"] - row[f"embed_{tag}"]["median_ms"]
    eng.profile(True)
    eng.embed_tokens(pix, offs, hw, 0, out=tok, out_f32=e32, out_bf16=e16)
    prof = eng.profile_read()
    eng.profile(False)
    row["class_ms_token_pass"] = {k: v[0] for k, v in prof.items() if v[1]}
    # the token kernel's own traffic: the window's residual rows read, the token rows written
    row["token_kernel_algorithmic_bytes"] = 2 * n * ntok * d * 2
    # what the token kernel would take at the HBM peak, beside the measured extra time over the full pass
    row["token_kernel_ms_at_hbm_peak"] = row["token_kernel_algorithmic_bytes"] / (HBM_PEAK_GBS * 1e9) * 1e3
    row["hbm_frac_of_extra_full"] = row["token_kernel_ms_at_hbm_peak"] / row["extra_ms_full"] if row["extra_ms_full"] > 0 else None
    if not bool(torch.isfinite(tok.float()).all()):
        raise SystemExit(f"{name}: non-finite token rows")
    eng.close()
    print(f"{name:10s} n {n}: embed {row['embed_full']['median_ms']:.3f} ms (pruned {row['embed_pruned']['median_ms']:.3f}), with tokens "
          f"{row['embed_tokens_full']['median_ms']:.3f} ms (pruned setting {row['embed_tokens_pruned']['median_ms']:.3f}): + {row['extra_ms_full']:.3f} ms "
          f"over the full pass, + {row['extra_ms_pruned']:.3f} ms over the pruned one; {row['token_bytes'] / 1e6:.1f} MB of token rows", flush=True)
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokens.json"))
    args = ap.parse_args(argv)
    if min(args.crops, args.steps) < 1 or args.warmup < 0:
        ap.error("counts and --steps must be positive, --warmup non-negative")

    import torch

    from multimodal_embeddings_amd.build import kernel_source_hash

    if not torch.cuda.is_available():
        raise SystemExit("bench_tokens: no GPU visible; this is a GPU measurement and has no fallback")
    result = {"tool": "bench_tokens", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "steps": args.steps,
              "warmup": args.warmup, "hbm_peak_gb_per_s": HBM_PEAK_GBS,
              "token_pass": [token_pass(name, args) for name in ("vit_b16", "dinov2_b14")]}
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
        print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
