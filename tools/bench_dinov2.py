#!/usr/bin/env python3
"""The patch-14 pass beside the patch-16 pass: seeded DINOv2-B/14 and ViT-B/16 on the same crops in one process.

    python tools/bench_dinov2.py [--crops 48,4096] [--steps 7] [--warmup 3] [--out FILE]

For each crop count n (chunk = n) and each of the two towers: `--warmup` untimed and `--steps` timed calls of mme_embed
(K1 + the whole forward; at patch 14 K1 -> retile_patches_p14 -> pass), every timed call between its own pair of HIP
events: median and range.  Then one more call under mme_profile_enable: kernel time by class.  At patch 14 the class
"attention" is attn_mid alone (12 launches at B/14), "preprocess" is K1 + retile_patches_p14 and "layernorm" includes
embed_rows at 257 tokens.  The kernels the patch-14 path adds are also timed alone through mme_dinov2_apply (median of
`--steps` synchronous launches, so each figure includes one launch + synchronise round trip, printed beside it as the time
of an n = 0 launch): the retile, embed_rows, and ONE attention launch, whose achieved bytes per second is quoted against
its algorithmic traffic of 257 x 4 x 128 B per (crop, head) item (Q, K, V read and the output written once).  Prints a
table and ONE JSON line (DESIGN.md 4.19 quotes it).  Needs a GPU; no fallback.
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


def timed(torch, fn, steps):
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def measure(name, geom, pix, offs, hw, args):
    import torch

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import dinov2_flops_per_crop, make_dinov2_weights, make_vit_weights, vit_flops_per_crop

    p14 = geom.patch_size == 14
    eng = Engine(0)
    if p14:
        eng.load_dinov2(make_dinov2_weights(1, geom), geom)
    else:
        eng.load_vit(make_vit_weights(1, geom), geom=geom)
    n, d = len(offs), eng.embed_dim
    eng.set_chunk(n)
    e32 = torch.empty((n, d), dtype=torch.float32, device=pix.device)
    e16 = torch.empty((n, d), dtype=torch.bfloat16, device=pix.device)
    run = lambda: eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16)  # noqa: E731
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    row = {"name": name, "patch": geom.patch_size, "crops": n, "flop_per_crop": dinov2_flops_per_crop(geom) if p14 else vit_flops_per_crop(geom)}
    row.update(timed(torch, run, args.steps))
    row["crops_per_s"] = n / (row["median_ms"] * 1e-3)
    eng.profile(True)
    run()
    row["class_ms"] = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
    row["class_launches"] = {k: v[1] for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)
    if not bool(torch.isfinite(e32).all()):
        raise SystemExit(f"{name}: non-finite embeddings")
    if p14:
        g = torch.Generator(device=pix.device).manual_seed(1)
        D, H = geom.hidden_size, geom.num_heads
        p16 = torch.randn((n * 196, 768), generator=g, device=pix.device).to(torch.bfloat16)
        pm = torch.empty((n * 256, 640), dtype=torch.bfloat16, device=pix.device)
        acc = torch.empty((n * 256, D), dtype=torch.float32, device=pix.device)
        tab = torch.randn((257 + 2, D), generator=g, device=pix.device)
        x = torch.empty((n * 257, D), dtype=torch.bfloat16, device=pix.device)
        qkv = (torch.randn((n * 257, 3 * D), generator=g, device=pix.device) * 0.5).to(torch.bfloat16)
        row["launch_sync_ms"] = timed(torch, lambda: eng.dinov2_apply("retile", src=p16, dst=pm, n=0), args.steps)["median_ms"]
        row["retile_patches_p14_ms"] = timed(torch, lambda: eng.dinov2_apply("retile", src=p16, dst=pm, n=n), args.steps)["median_ms"]
        row["embed_rows_t257_ms"] = timed(torch, lambda: eng.dinov2_apply("embed_rows", acc=acc, bias=tab[257], pos=tab[:257], cls=tab[258], x=x, n=n, d=D),
                                          args.steps)["median_ms"]
        row["attn_mid_ms"] = timed(torch, lambda: eng.dinov2_apply("attention", qkv=qkv, out=x, n=n, heads=H), args.steps)["median_ms"]
        row["attn_mid_algorithmic_bytes"] = n * H * 257 * 4 * 128
        net = max(row["attn_mid_ms"] - row["launch_sync_ms"], 1e-6)
        row["attn_mid_tb_per_s"] = row["attn_mid_algorithmic_bytes"] / (net * 1e-3) / 1e12
        row["attn_mid_tflops"] = n * H * 4 * 257 * 257 * 64 / (net * 1e-3) / 1e12
    eng.close()
    cls = "  ".join(f"{k} {v:.3f}" for k, v in row["class_ms"].items())
    print(f"{name:10s} n {n:5d}  median {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  {row['crops_per_s']:10.0f} crops/s  | by class: {cls}",
          flush=True)
    if p14:
        print(f"{'':10s} alone (launch + sync {row['launch_sync_ms']:.3f} ms included): retile {row['retile_patches_p14_ms']:.3f} ms, embed_rows "
              f"{row['embed_rows_t257_ms']:.3f} ms, attention {row['attn_mid_ms']:.3f} ms = {row['attn_mid_tb_per_s']:.3f} TB/s of algorithmic traffic, "
              f"{row['attn_mid_tflops']:.1f} TFLOP/s", flush=True)
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--crops", default="48,4096")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    counts = [int(v) for v in args.crops.split(",")]
    if min(counts) < 1 or args.steps < 1 or args.warmup < 0:
        ap.error("--crops and --steps must be positive, --warmup non-negative")

    import numpy as np
    import torch

    from multimodal_embeddings_amd.build import kernel_source_hash
    from multimodal_embeddings_amd.weights import DINOV2_B14, VIT_B16, synthetic_crops

    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov2: no GPU visible; this is a GPU measurement and has no fallback")
    dev = torch.device("cuda:0")
    rows = []
    for n in counts:
        pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
        for b0 in range(0, n, 4096):
            blk = synthetic_crops(min(4096, n - b0), seed=0, start=b0)
            pix[b0 * 150528 : (b0 + len(blk)) * 150528] = torch.from_numpy(blk.reshape(-1)).to(dev)
        offs = np.arange(n, dtype=np.int64) * 150528
        hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
        for name, geom in (("dinov2_b14", DINOV2_B14), ("vit_b16", VIT_B16)):
            rows.append(measure(name, geom, pix, offs, hw, args))
        del pix
    result = {"tool": "bench_dinov2", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "steps": args.steps,
              "warmup": args.warmup, "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
