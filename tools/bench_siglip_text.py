#!/usr/bin/env python3
"""The SigLIP text tower's time: SigLIP-B's text tower (768 x 12, vocabulary 32000, seeded) on n = 1, 48 and 4096 sequences.

    python tools/bench_siglip_text.py [--sizes 1,48,4096] [--repeats 7] [--warmup 3] [--cpu-max 48] [--out profiles/siglip_text_bench.txt]

Per size: `--warmup` untimed calls of Engine.text_forward (host id check, the id upload and the whole pass), then
`--repeats` calls timed one by one between two HIP events with a device synchronise in front; reported are the median
and the range of the repeats, sequences per second at the median, and the FLOP rate from
weights.siglip_text_flops_per_sequence as a fraction of the nominal 2.5 PFLOP/s dense bf16 peak (an end-to-end figure).
One further pass per size runs with the library's per-class event timing on and reports the kernel time by class
(attention = the 64-token attention kernel).  Beside it, for sizes up to `--cpu-max`, the time transformers' SiglipTextModel takes for the same ids in
float32 on this host's CPU (median of three calls after one warm-up), with the number of cores torch uses: a reference
point for what the call replaces, not a like-for-like race.  Nothing here is gated: there is no earlier figure.
Prints a table and ONE JSON line, and writes both to --out.  Needs a GPU; no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

NOMINAL_FLOPS = 2.5e15


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="1,48,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-max", type=int, default=48, help="largest size the transformers CPU reference is timed at (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siglip_text_bench.txt"))
    args = ap.parse_args(argv)
    sizes = [int(v) for v in args.sizes.split(",")]
    if min(sizes) < 1 or args.repeats < 1 or args.warmup < 0:
        ap.error("--sizes and --repeats must be positive, --warmup non-negative")

    import numpy as np
    import torch

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.build import kernel_source_hash
    from multimodal_embeddings_amd.weights import SIGLIP_TEXT_B, make_siglip_text_weights, siglip_text_flops_per_sequence, siglip_token_ids

    if not torch.cuda.is_available():
        raise SystemExit("bench_siglip_text: no GPU visible; this is a GPU measurement and has no fallback")
    geom = SIGLIP_TEXT_B
    w = make_siglip_text_weights(5, geom)
    eng = Engine(0)
    eng.load_siglip_text(w, geom)
    flop = siglip_text_flops_per_sequence(geom)
    model = None
    if args.cpu_max:
        try:
            import make_siglip_text_golden as mk

            model = mk.hf_text_model(geom, w)
        except ImportError as e:
            print(f"transformers is not importable ({e}): no CPU reference", flush=True)
    lines = [f"bench_siglip_text: SigLIP-B text tower {geom.hidden_size} x {geom.num_layers}, vocab {geom.vocab_size}, {flop / 1e9:.3f} GFLOP / sequence, "
             f"device {torch.cuda.get_device_name(0)}, warm-up {args.warmup}, repeats {args.repeats}, CPU reference on {torch.get_num_threads()} cores"]
    rows = []
    for n in sizes:
        ids = siglip_token_ids(n, geom.vocab_size, geom.pad_token_id, 1)
        for _ in range(args.warmup):
            e32, _ = eng.text_forward(ids, want_bf16=False)
        ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e32, _ = eng.text_forward(ids, want_bf16=False)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        if not bool(torch.isfinite(e32).all()):
            raise SystemExit(f"n = {n}: non-finite embeddings")
        med = statistics.median(ms)
        # one more pass with the library's per-class event timing on: where the time goes (the text pass files its launches under the
        # image pass's classes: preprocess = token rows, layernorm = the statistics passes, pool = last-row pool-LN + bias + L2)
        eng.profile(True)
        eng.text_forward(ids, want_bf16=False)
        prof = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
        eng.profile(False)
        total = sum(prof.values()) or 1.0
        row = {"n": n, "kernel_ms_by_class": prof, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "sequences_per_s": n / (med * 1e-3),
               "frac_of_nominal": flop * n / (med * 1e-3) / NOMINAL_FLOPS, "cpu_ms_median": None, "one_minus_cos_vs_cpu": None}
        if model is not None and n <= args.cpu_max:
            t = torch.from_numpy(ids.astype(np.int64))
            cpu = []
            with torch.no_grad():
                ref = model(input_ids=t).pooler_output
                for _ in range(3):
                    t0 = time.perf_counter()
                    model(input_ids=t)
                    cpu.append((time.perf_counter() - t0) * 1e3)
            row["cpu_ms_median"] = statistics.median(cpu)
            r, g = ref.double().numpy(), e32.double().cpu().numpy()
            row["one_minus_cos_vs_cpu"] = float((1.0 - (r * g).sum(1) / np.linalg.norm(r, axis=1) / np.linalg.norm(g, axis=1)).max())
        rows.append(row)
        cpu_txt = "" if row["cpu_ms_median"] is None else f"  transformers f32 CPU {row['cpu_ms_median']:9.1f} ms  max(1 - cos) {row['one_minus_cos_vs_cpu']:.2g}"
        lines.append(f"n {n:5d}  median {med:9.3f} ms  range {min(ms):9.3f} .. {max(ms):9.3f}  {row['sequences_per_s']:10.0f} seq/s  "
                     f"{row['frac_of_nominal']:.4f} of nominal{cpu_txt}")
        print(lines[-1], flush=True)
        lines.append("         kernel time by class: " + ", ".join(f"{k} {v:.3f} ms ({100 * v / total:.0f} %)" for k, v in prof.items()))
        print(lines[-1], flush=True)
    eng.close()
    result = {"tool": "bench_siglip_text", "device": torch.cuda.get_device_name(0), "kernel_source_hash": kernel_source_hash(), "geometry": str(geom),
              "flop_per_sequence": flop, "warmup": args.warmup, "repeats": args.repeats, "cpu_threads": torch.get_num_threads(), "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
