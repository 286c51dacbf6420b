#!/usr/bin/env python3
"""The patch-32 pass beside the patch-16 pass: seeded CLIP-B/32 and CLIP-B/16 on the same crops in one process.

    python tools/bench_vit32.py [--crops 48,4096] [--steps 7] [--warmup 3] [--out FILE]

For each crop count n (chunk = n) and each of the two towers: `--warmup` untimed and `--steps` timed calls of mme_embed
(K1 + the whole forward; at patch 32 K1 -> retile_patches_p32 -> pass), every timed call between its own pair of HIP
events: median and range.  Then one more call under mme_profile_enable: kernel time by class.  At patch 32 the class
"attention" is attn_short<50> alone, "preprocess" is K1 + retile_patches_p32 and "layernorm" includes embed_rows_t50; the
two kernels the patch-32 path adds in front of the encoder are also timed alone through mme_vit32_apply (median of
`--steps` synchronous launches, so each figure includes one launch + synchronise round trip, printed beside it as the
time of an n = 0 launch), and the f32 patch-embed GEMM [49 n, 3072] x [3072, 768] through mme_gemm_apply, beside the
patch-16 tower's fused one.  Prints a table and ONE JSON line (DESIGN.md 4.10 quotes it).  Needs a GPU; no fallback.
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
    from multimodal_embeddings_amd.weights import clip_flops_per_crop, make_clip_weights

    eng = Engine(0)
    eng.load_clip(make_clip_weights(1, geom), geom)
    n, d = len(offs), eng.embed_dim
    eng.set_chunk(n)
    e32 = torch.empty((n, d), dtype=torch.float32, device=pix.device)
    e16 = torch.empty((n, d), dtype=torch.bfloat16, device=pix.device)
    run = lambda: eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16)  # noqa: E731
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    row = {"name": name, "patch": geom.patch_size, "crops": n, "flop_per_crop": clip_flops_per_crop(geom)}
    row.update(timed(torch, run, args.steps))
    row["crops_per_s"] = n / (row["median_ms"] * 1e-3)
    eng.profile(True)
    run()
    row["class_ms"] = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
    row["class_launches"] = {k: v[1] for k, v in eng.profile_read().items() if v[1]}
    eng.profile(False)
    if not bool(torch.isfinite(e32).all()):
        raise SystemExit(f"{name}: non-finite embeddings")
    g = torch.Generator(device=pix.device).manual_seed(1)
    D = geom.hidden_size
    if geom.patch_size == 32:
        p16 = torch.randn((n * 196, 768), generator=g, device=pix.device).to(torch.bfloat16)
        p32 = torch.empty((n * 49, 3072), dtype=torch.bfloat16, device=pix.device)
        acc = torch.empty((n * 49, D), dtype=torch.float32, device=pix.device)
        tab = torch.randn((50 + 2, D), generator=g, device=pix.device)
        x = torch.empty((n * 50, D), dtype=torch.bfloat16, device=pix.device)
        W = torch.randn((D, 3072), generator=g, device=pix.device).to(torch.bfloat16)
        row["launch_sync_ms"] = timed(torch, lambda: eng.vit32_apply("retile", src=p16, dst=p32, n=0), args.steps)["median_ms"]
        row["retile_patches_p32_ms"] = timed(torch, lambda: eng.vit32_apply("retile", src=p16, dst=p32, n=n), args.steps)["median_ms"]
        row["embed_rows_t50_ms"] = timed(torch, lambda: eng.vit32_apply("embed_rows", acc=acc, bias=tab[50], pos=tab[:50], cls=tab[51], x=x, n=n, d=D),
                                         args.steps)["median_ms"]
        row["patch_embed_gemm_f32_ms"] = timed(torch, lambda: eng.gemm_apply(4, p32, W, outf=acc), args.steps)["median_ms"]
    else:
        p16 = torch.randn((n * 196, 768), generator=g, device=pix.device).to(torch.bfloat16)
        W = torch.randn((D, 768), generator=g, device=pix.device).to(torch.bfloat16)
        tab = torch.randn((197 + 1, D), generator=g, device=pix.device)
        x = torch.empty((n * 197, D), dtype=torch.bfloat16, device=pix.device)
        row["launch_sync_ms"] = timed(torch, lambda: eng.vit32_apply("retile", src=p16, dst=x, n=0), args.steps)["median_ms"]
        row["patch_embed_gemm_fused_ms"] = timed(torch, lambda: eng.gemm_apply(3, p16, W, bias=tab[197], pos=tab[:197], out=x), args.steps)["median_ms"]
    eng.close()
    cls = "  ".join(f"{k} {v:.3f}" for k, v in row["class_ms"].items())
    print(f"{name:10s} n {n:5d}  median {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  {row['crops_per_s']:10.0f} crops/s  | by class: {cls}",
          flush=True)
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
    from multimodal_embeddings_amd.weights import CLIP_B16, CLIP_B32, synthetic_crops

    if not torch.cuda.is_available():
        raise SystemExit("bench_vit32: no GPU visible; this is a GPU measurement and has no fallback")
    dev = torch.device("cuda:0")
    rows = []
    for n in counts:
        pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
        for b0 in range(0, n, 4096):
            blk = synthetic_crops(min(4096, n - b0), seed=0, start=b0)
            pix[b0 * 150528 : (b0 + len(blk)) * 150528] = torch.from_numpy(blk.reshape(-1)).to(dev)
        offs = np.arange(n, dtype=np.int64) * 150528
        hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
        for name, geom in (("clip_b32", CLIP_B32), ("clip_b16", CLIP_B16)):
            rows.append(measure(name, geom, pix, offs, hw, args))
        del pix
    result = {"tool": "bench_vit32", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "steps": args.steps,
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
