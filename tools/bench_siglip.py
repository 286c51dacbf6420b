#!/usr/bin/env python3
"""The SigLIP pass beside the CLIP pass: seeded SigLIP-B/16 and CLIP-B/16 on the same crops in one process.

    python tools/bench_siglip.py [--crops 48,4096] [--steps 7] [--warmup 3] [--out FILE]

For each crop count n (chunk = n) and each of the two towers: `--warmup` untimed and `--steps` timed calls of mme_embed
(K1 + the whole forward), every timed call between its own pair of HIP events: median and range.  Then one more call under
mme_profile_enable: kernel time by class.  Under SigLIP the class "layernorm" includes embed_rows_t196 and "pool" is
map_pool + the zeroing of the head's residual rows + l2_rows_bf16; the head's GEMMs are in "gemm".  The parts the tower adds
are also timed alone (median of `--steps` synchronous launches, so each figure includes one launch + synchronise round
trip, printed beside it as the time of an n = 0 launch):
  the head      the K | V GEMM [196 n, D] x [D, 2 D] with the folded LayerNorm (mme_gemm_apply, epilogue 5), map_pool, and the tail
                on n rows: out_proj (epilogue 2), fc1 with tanh-GELU (mme_siglip_apply op 1), fc2 (epilogue 2), l2_rows_bf16
  the detour    the f32 patch-embed GEMM [196 n, 768] x [768, D] (epilogue 4) + embed_rows_t196, beside CLIP's fused one (epilogue 3)
Prints a table and ONE JSON line (DESIGN.md 4.15 quotes it).  Needs a GPU; no fallback.
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
    from multimodal_embeddings_amd.weights import clip_flops_per_crop, make_clip_weights, make_siglip_weights, siglip_flops_per_crop

    siglip = name.startswith("siglip")
    eng = Engine(0)
    if siglip:
        eng.load_siglip(make_siglip_weights(1, geom), geom)
    else:
        eng.load_clip(make_clip_weights(1, geom), geom)
    n, d = len(offs), eng.embed_dim
    eng.set_chunk(n)
    e32 = torch.empty((n, d), dtype=torch.float32, device=pix.device)
    e16 = torch.empty((n, d), dtype=torch.bfloat16, device=pix.device)
    run = lambda: eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16)  # noqa: E731
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    row = {"name": name, "crops": n, "flop_per_crop": siglip_flops_per_crop(geom) if siglip else clip_flops_per_crop(geom)}
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
    D, F, H = geom.hidden_size, geom.intermediate_size, geom.num_heads
    bf, f32 = torch.bfloat16, torch.float32
    rnd = lambda shape, dt=bf: torch.randn(shape, generator=g, device=pix.device).to(dt)  # noqa: E731
    med = lambda fn: timed(torch, fn, args.steps)["median_ms"]  # noqa: E731
    p16, Wp = rnd((n * 196, 768)), rnd((D, 768))
    if siglip:
        x, acc = rnd((n * 196, D)), torch.empty((n * 196, D), dtype=f32, device=pix.device)
        pos, vec = rnd((196, D), f32), rnd((8, 2 * D), f32)
        st = torch.zeros((n * 196, 2), dtype=f32, device=pix.device)
        st[:, 1] = 1.0
        kv, Wkv = torch.empty((n * 196, 2 * D), dtype=bf, device=pix.device), rnd((2 * D, D)) * 0.05
        a, y, m = torch.empty((n, D), dtype=bf, device=pix.device), torch.zeros((n, D), dtype=bf, device=pix.device), torch.empty((n, F), dtype=bf, device=pix.device)
        Wo, W1, W2 = rnd((D, D)) * 0.05, rnd((F, D)) * 0.05, rnd((D, F)) * 0.05
        b1, cs1 = rnd((F,), f32), torch.zeros((F,), dtype=f32, device=pix.device)
        row["launch_sync_ms"] = med(lambda: eng.siglip_apply("map_pool", kv=kv, q=vec[0, :D], out=a, n=0, heads=H))
        row["head_kv_gemm_ms"] = med(lambda: eng.gemm_apply(5, x, Wkv, bias=vec[1], out=kv, ln_stats=st, colsum=vec[2]))
        row["head_map_pool_ms"] = med(lambda: eng.siglip_apply("map_pool", kv=kv, q=vec[0, :D], out=a, n=n, heads=H))
        row["head_out_proj_ms"] = med(lambda: eng.gemm_apply(2, a, Wo, bias=vec[3, :D], out=y, res=y))
        row["head_fc1_tgelu_ms"] = med(lambda: eng.siglip_apply("gemm_ln_tgelu", A=y, W=W1, bias=b1, out=m, ln_stats=st[:n], colsum=cs1))
        row["head_fc2_ms"] = med(lambda: eng.gemm_apply(2, m, W2, bias=vec[4, :D], out=y, res=y))
        row["head_l2_rows_bf16_ms"] = med(lambda: eng.siglip_apply("l2_bf16", x=y, emb_f32=e32, n=n, d=D))
        row["patch_embed_gemm_f32_ms"] = med(lambda: eng.gemm_apply(4, p16, Wp, outf=acc))
        row["embed_rows_t196_ms"] = med(lambda: eng.siglip_apply("embed_rows", acc=acc, bias=vec[5, :D], pos=pos, x=x, n=n, d=D))
    else:
        tab = rnd((197 + 1, D), f32)
        x = torch.empty((n * 197, D), dtype=bf, device=pix.device)
        row["launch_sync_ms"] = med(lambda: eng.siglip_apply("map_pool", kv=p16, q=tab[0], out=x, n=0, heads=H))
        row["patch_embed_gemm_fused_ms"] = med(lambda: eng.gemm_apply(3, p16, Wp, bias=tab[197], pos=tab[:197], out=x))
    eng.close()
    cls = "  ".join(f"{k} {v:.3f}" for k, v in row["class_ms"].items())
    print(f"{name:11s} n {n:5d}  median {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  {row['crops_per_s']:10.0f} crops/s  | by class: {cls}",
          flush=True)
    alone = "  ".join(f"{k[:-3]} {v:.3f}" for k, v in row.items() if k.endswith("_ms") and k not in ("median_ms", "min_ms", "max_ms", "class_ms"))
    print(f"{'':11s} alone (ms): {alone}", flush=True)
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
    from multimodal_embeddings_amd.weights import CLIP_B16, SIGLIP_B16, synthetic_crops

    if not torch.cuda.is_available():
        raise SystemExit("bench_siglip: no GPU visible; this is a GPU measurement and has no fallback")
    dev = torch.device("cuda:0")
    rows = []
    for n in counts:
        pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
        for b0 in range(0, n, 4096):
            blk = synthetic_crops(min(4096, n - b0), seed=0, start=b0)
            pix[b0 * 150528 : (b0 + len(blk)) * 150528] = torch.from_numpy(blk.reshape(-1)).to(dev)
        offs = np.arange(n, dtype=np.int64) * 150528
        hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
        for name, geom in (("siglip_b16", SIGLIP_B16), ("clip_b16", CLIP_B16)):
            rows.append(measure(name, geom, pix, offs, hw, args))
        del pix
    result = {"tool": "bench_siglip", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "steps": args.steps,
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
