#!/usr/bin/env python3
"""Per-shape GEMM A/B (random bf16 data on the device), the kernel variants INTERLEAVED in one process.

    python tools/gemm_bench.py [--arms 4,6] [--rounds 5] [--iters 3] [--rows 806912] [--json out.json]

The four GEMMs of a ViT-B/16 block at chunk = 4096 crops, each with the epilogue the forward runs it with (folded
LayerNorm for QKV and fc1, residual + statistics planes for o_proj and fc2).  A round times `iters` synchronous launches
of every arm in turn; per arm the median and minimum over the rounds and the round-to-round spread (max - min) are
printed, and the verdict the variant table of gemm.hip goes by: the last arm beats the first when its median is lower by
more than the first arm's own spread.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multimodal_embeddings_amd._lib import Engine

SHAPES = [  # (name, N, K, epilogue)
    ("qkv", 2304, 768, 5),
    ("proj", 768, 768, 8),
    ("fc1", 3072, 768, 6),
    ("fc2", 768, 3072, 8),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="4,6")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=806912)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    arms = [int(a) for a in args.arms.split(",")]
    M = args.rows
    eng = Engine(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda shape, scale, dtype: (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)  # noqa: E731
    record = []
    for name, N, K, epi in SHAPES:
        A, W = rnd((M, K), 1.0, torch.bfloat16), rnd((N, K), 0.05, torch.bfloat16)
        out = rnd((M, N), 1.0, torch.bfloat16)
        kw = dict(bias=rnd((N,), 0.5, torch.float32), out=out, ldo=N)
        if epi == 8:
            kw.update(res=out, ln_part=torch.empty(2 * (N // 64) * M, dtype=torch.float32, device="cuda"), ln_part_rows=M)
        else:
            stats = torch.stack([rnd((M,), 0.1, torch.float32), 1.0 + rnd((M,), 0.1, torch.float32).abs()], dim=1).contiguous()
            kw.update(ln_stats=stats, colsum=rnd((N,), 0.5, torch.float32))
        ms = {a: [] for a in arms}
        for r in range(args.rounds + 1):  # round 0 warms up
            for a in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    eng.gemm_apply(epi, A, W, variant=a, **kw)
                dt = (time.perf_counter() - t0) / args.iters * 1e3
                if r:
                    ms[a].append(dt)
        row = {"shape": name, "M": M, "N": N, "K": K, "epilogue": epi, "arms": {}}
        for a in arms:
            t = sorted(ms[a])
            row["arms"][str(a)] = {"ms": ms[a], "median": t[len(t) // 2], "min": t[0], "spread": t[-1] - t[0]}
            print(f"{name:5s} v{a}: ms med {t[len(t) // 2]:.4f} min {t[0]:.4f} spread {t[-1] - t[0]:.4f}  TF/s at the median {2.0 * M * N * K / t[len(t) // 2] / 1e9:.0f}", flush=True)
        first, last = row["arms"][str(arms[0])], row["arms"][str(arms[-1])]
        row["last_arm_wins"] = bool(first["median"] - last["median"] > first["spread"])
        print(f"{name:5s} v{arms[-1]} - v{arms[0]}: {last['median'] - first['median']:+.4f} ms at the median; v{arms[-1]} wins: {row['last_arm_wins']}", flush=True)
        record.append(row)
        del A, W, out, kw
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
