#!/usr/bin/env python3
"""Mean pooling over the covered patches, measured in one fresh process.

    python tools/bench_pool.py [--crops 4096] [--steps 9] [--warmup 3] [--out profiles/pooling.json]

1. The pooling launch alone (mme_pool_apply on a seeded residual stream, ViT-B/16: 197 tokens of 768) at `--crops` crops: whole
   grids, then the covered grids of the bundled crop shapes (tests/golden/bundled_crop_sizes_hw.npy, repeated to `--crops`), both
   ops; beside it K8 (mme_rowop_apply, pool_ln_l2) at the same count.  Each as time and as a fraction of the time the HBM peak
   needs for the bytes the launch must read (the covered rows, 1536 bytes each).  The hooks synchronise the stream before they
   return, so an event pair around one call holds the kernel and the few microseconds until the host has recorded the second event.
2. Whole mme_embed on 224 x 224 crops in one chunk, forward pruning off: pooling "token" against "mean" and "cls+mean".
Every timed call sits between its own pair of HIP events behind `--warmup` untimed calls: median and range.  Prints a table and
writes ONE JSON document.  Needs a GPU; no fallback.
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
TOKENS, G, D = 197, 14, 768


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


def with_peak(row, rows_read):
    row["bytes_read"] = int(rows_read) * D * 2
    row["ms_at_hbm_peak"] = row["bytes_read"] / (HBM_PEAK_GBS * 1e9) * 1e3
    row["hbm_frac"] = row["ms_at_hbm_peak"] / row["median_ms"]
    return row


def launches(args):
    import numpy as np
    import torch

    from multimodal_embeddings_amd._lib import Engine

    dev = torch.device("cuda:0")
    n = args.crops
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n * TOKENS, D), generator=g, device=dev).to(torch.bfloat16)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g, device=dev)
    beta = 0.5 * torch.randn(D, generator=g, device=dev)
    hw = np.load(os.path.join(ROOT, "tests", "golden", "bundled_crop_sizes_hw.npy"))
    covered = np.array([Engine.pool_grid(int(h), int(w), 16) for h, w in hw], dtype=np.int32)
    covered = covered[np.arange(n) % len(covered)]
    grids = {"whole": None, "bundled": torch.from_numpy(covered).to(dev)}
    rows = {"whole": n * G * G, "bundled": int((covered[:, 0].astype(np.int64) * covered[:, 1]).sum())}
    eng = Engine(0)
    out = {"crops": n, "tokens": TOKENS, "hidden": D, "bundled_mean_share_of_patches": rows["bundled"] / rows["whole"]}
    for op in ("mean", "cls+mean"):
        E = D * (2 if op == "cls+mean" else 1)
        e32 = torch.empty((n, E), dtype=torch.float32, device=dev)
        e16 = torch.empty((n, E), dtype=torch.bfloat16, device=dev)
        for name, G_dev in grids.items():
            a = _args(eng, x, gamma, beta, G_dev, e32, e16, n)  # (Engine.pool_apply would re-check the device grids inside every timed call)
            opcode = eng.POOL_OPS[op]
            call = lambda: eng._check(eng.lib.mme_pool_apply(eng.h, opcode, a, eng._stream()), "mme_pool_apply")  # noqa: E731
            row = with_peak(timed(torch, call, args.steps, args.warmup), rows[name] + (n if op == "cls+mean" else 0))
            out[f"{op}_{name}"] = row
            print(f"pool_apply {op:8s} {name:7s} n {n}: {row['median_ms']:.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f}); "
                  f"{row['bytes_read'] / 1e6:.0f} MB read, {row['hbm_frac']:.2f} of the HBM peak", flush=True)
            if not bool(torch.isfinite(e32).all()):
                raise SystemExit(f"{op} {name}: non-finite output")
    k32 = torch.empty((n, D), dtype=torch.float32, device=dev)
    k16 = torch.empty((n, D), dtype=torch.bfloat16, device=dev)
    row = with_peak(timed(torch, lambda: eng.rowop_apply("pool_ln_l2", x=x, gamma=gamma, beta=beta, B=n, tok=0, d=D, emb_f32=k32, emb_bf16=k16),
                          args.steps, args.warmup), n)
    out["k8_pool_ln_l2"] = row
    print(f"rowop_apply pool_ln_l2 (K8) n {n}: {row['median_ms']:.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f})", flush=True)
    eng.close()
    return out


def _args(eng, x, gamma, beta, grids, e32, e16, n):
    import ctypes as C

    from multimodal_embeddings_amd._lib import _PoolApplyArgs

    a = _PoolApplyArgs()
    a.x, a.gamma, a.beta, a.grids, a.emb_f32, a.emb_bf16 = (eng._ptr(t) for t in (x, gamma, beta, grids, e32, e16))
    a.B, a.tokens, a.g, a.first, a.d, a.eps = n, TOKENS, G, 1, D, 1e-12
    return C.byref(a)


def whole_embed(args):
    import numpy as np
    import torch

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import VIT_B16, make_vit_weights, synthetic_crops

    dev = torch.device("cuda:0")
    n = args.crops
    pix = torch.empty(n * 150528 + 16, dtype=torch.uint8, device=dev)
    pix[: n * 150528] = torch.from_numpy(synthetic_crops(n, seed=0).reshape(-1)).to(dev)
    offs = np.arange(n, dtype=np.int64) * 150528
    hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
    eng = Engine(0)
    eng.load_vit(make_vit_weights(1, VIT_B16), geom=VIT_B16)
    eng.set_chunk(n)
    eng.set_forward_pruning(False)
    out = {"crops": n, "encoder": "vit_b16", "pruning": False}
    for mode in ("token", "mean", "cls+mean", "token"):
        eng.set_pooling(mode)
        E = eng.embed_dim
        e32 = torch.empty((n, E), dtype=torch.float32, device=dev)
        e16 = torch.empty((n, E), dtype=torch.bfloat16, device=dev)
        row = timed(torch, lambda: eng.embed(pix, offs, hw, 0, out_f32=e32, out_bf16=e16), args.steps, args.warmup)
        out[mode if mode not in out else mode + "_again"] = row
        print(f"mme_embed pooling {mode:8s} n {n}: {row['median_ms']:.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f})", flush=True)
        if not bool(torch.isfinite(e32).all()):
            raise SystemExit(f"mme_embed {mode}: non-finite output")
    eng.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--crops", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooling.json"))
    args = ap.parse_args(argv)
    if min(args.crops, args.steps) < 1 or args.warmup < 0:
        ap.error("--crops and --steps must be positive, --warmup non-negative")

    import torch

    from multimodal_embeddings_amd.build import kernel_source_hash

    if not torch.cuda.is_available():
        raise SystemExit("bench_pool: no GPU visible; this is a GPU measurement and has no fallback")
    result = {"tool": "bench_pool", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "steps": args.steps,
              "warmup": args.warmup, "hbm_peak_gb_per_s": HBM_PEAK_GBS, "launch": launches(args), "embed": whole_embed(args)}
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
        print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
