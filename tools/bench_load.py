#!/usr/bin/env python3
"""Load time: context creation -> weights ready, host preparation against device preparation.

    python tools/bench_load.py [--encoders vit_b16,mllama_tiles] [--tile-layers 32,8] [--out profiles/load_times.json]

For each encoder three cases, each in a FRESH child process (one warm-up load, three timed loads, median):
    host_f32    Engine.load_vit / load_tile_vit from the f32 dict: every tensor prepared by the host loops, then uploaded
    dev_f32     Engine.load_*_checkpoint from the same weights as an f32 checkpoint: raw bytes copied, prepared by kernels
    dev_bf16    the same from a bf16 checkpoint (half the bytes)
The parent generates the seeded weights once, writes them as two checkpoint directories under a temporary directory and
needs no GPU itself.  A timed load is `Engine(0)` + load + device synchronisation; the weights are in host memory before
the clock starts (reading the file is not part of it).  Prints a table and ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ("host_f32", "dev_f32", "dev_bf16")


def child(encoder: str, case: str, directory: str) -> None:
    import torch

    from multimodal_embeddings_amd import checkpoint as ckpt
    from multimodal_embeddings_amd._lib import Engine

    ck = ckpt.read_checkpoint(directory, encoder)
    host = {k: t.float().numpy() for k, t in ck.tensors.items()} if case == "host_f32" else None
    copied = ck.nbytes if host is None else None

    def load():
        t0 = time.perf_counter()
        e = Engine(0)
        if host is not None:
            e.load_vit(host, eps=ck.geometry.layer_norm_eps) if encoder == "vit_b16" else e.load_tile_vit(host, ck.geometry)
        else:
            e.load_vit_checkpoint(ck) if encoder == "vit_b16" else e.load_tile_vit_checkpoint(ck)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = len(e.weights_fingerprint())
        e.close()
        return dt, n

    load()
    runs = [load() for _ in range(3)]
    print(json.dumps({"encoder": encoder, "case": case, "dtype": ck.dtype, "median_s": statistics.median(r[0] for r in runs),
                      "runs_s": [round(r[0], 4) for r in runs], "buffers": runs[0][1], "checkpoint_bytes_copied": copied,
                      "tensors": len(ck.tensors)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--encoders", default="vit_b16,mllama_tiles")
    ap.add_argument("--tile-layers", default="32,8", help="local,global layers of the tile tower (32,8 = the full tower)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--child", nargs=3, metavar=("ENCODER", "CASE", "DIR"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return 0

    from multimodal_embeddings_amd import checkpoint as ckpt
    from multimodal_embeddings_amd.weights import TILE_VIT, TileViTGeometry, make_tile_vit_weights, make_vit_weights

    results = []
    with tempfile.TemporaryDirectory(prefix="mme_load_") as tmp:
        for encoder in a.encoders.split(","):
            if encoder == "vit_b16":
                geom, w = None, make_vit_weights(a.seed)
            else:
                nl, ng = (int(v) for v in a.tile_layers.split(","))
                inter = TILE_VIT.intermediate_layers if nl == 32 else tuple(range(0, nl, max(1, nl // 2)))[:2]
                geom = TileViTGeometry(num_layers=nl, num_global_layers=ng, intermediate_layers=inter)
                w = make_tile_vit_weights(a.seed, geom)
            dirs = {}
            for dtype in ("float32", "bfloat16"):
                dirs[dtype] = ckpt.save_checkpoint(os.path.join(tmp, f"{encoder}_{dtype}"), w, encoder, dtype, geom)
            del w
            print(f"{encoder}: checkpoints written", file=sys.stderr, flush=True)
            for case in CASES:
                d = dirs["bfloat16" if case == "dev_bf16" else "float32"]
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", encoder, case, d], capture_output=True, text=True,
                                   timeout=a.timeout)
                if r.returncode != 0:
                    print(r.stdout, r.stderr, sep="\n", file=sys.stderr)
                    print(f"{encoder} {case}: child exited with {r.returncode}; stopping", file=sys.stderr)
                    return 1
                results.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(f"{encoder} {case}: {results[-1]['median_s']:.3f} s", file=sys.stderr, flush=True)
                if encoder != "vit_b16":
                    results[-1]["layers"] = a.tile_layers
    print(f"{'encoder':14s} {'case':9s} {'median s':>9s}  {'runs s':28s} {'bytes copied':>13s}")
    for r in results:
        copied = "-" if r["checkpoint_bytes_copied"] is None else str(r["checkpoint_bytes_copied"])
        print(f"{r['encoder']:14s} {r['case']:9s} {r['median_s']:9.3f}  {str(r['runs_s']):28s} {copied:>13s}")
    line = json.dumps({"bench": "load", "seed": a.seed, "results": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
