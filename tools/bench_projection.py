#!/usr/bin/env python3
"""Timing of K17: the moments of the vector table and the projection of its rows, on seeded synthetic rows;
the record goes to profiles/projection.json.

    python tools/bench_projection.py [--out profiles/projection.json] [--torch-timeout 300]

Data: N = 65 536 unit bf16 rows of d = 768 with a common component (0.8 along one direction), a seeded f32 mean, and for
m = 64 / 256 / 768 a seeded f32 weight matrix of m orthonormal rows.  Three warm-up runs, seven timed ones, median and range,
every figure between two HIP events on the stream of the calls:
  moments          one mme_moments over the table (moments_block and moments_reduce)
  project_f32      one mme_project writing the f32 coordinates [N, m]
  project_bf16     one mme_project writing the normalised bf16 rows [N, m] (f32 rows through the workspace, then the row kernel)
The engine's figures are written first.  The torch yardstick then runs in a fresh child process under its own timeout -- float64
`x.T @ x` (and the column sums) of the widened table for the moments, float32 `(x - mean) @ W.T` then `normalize` for the
projection -- and is merged into the record when it comes back; if it does not, the record says so.  No figure is gated.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, RUNS = 3, 7
N, D, MS = 65536, 768, (64, 256, 768)


def table(torch, seed=17):
    """bf16 [N, D] unit rows 0.8 u + 0.6 v, the f32 mean 0.8 u, and f32 [D, D] orthonormal rows (the first m are the weights)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(D, generator=g, device="cuda"), dim=0)
    v = torch.nn.functional.normalize(torch.randn(N, D, generator=g, device="cuda"), dim=1)
    x = torch.nn.functional.normalize(0.8 * u + 0.6 * v, dim=1).to(torch.bfloat16)
    q = torch.linalg.qr(torch.randn(D, D, generator=g, device="cuda"))[0].t().contiguous()
    return x, (0.8 * u).contiguous(), q


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(torch, fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    return stats([event_ms(torch, fn) for _ in range(RUNS)])


def engine_part():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    x, mean, q = table(torch)
    rec = {"N": N, "d": D, "moments_block": Engine.MOMENTS_BLOCK, "moments_ms": timed(torch, lambda: eng.moments(x)), "project": []}
    for m in MS:
        w = q[:m].contiguous()
        y32 = torch.empty((N, m), dtype=torch.float32, device="cuda")
        rec["project"].append({"m": m, "project_f32_ms": timed(torch, lambda: eng.project(x, mean, w, normalise=False, out_f32=y32)),
                               "project_bf16_ms": timed(torch, lambda: eng.project(x, mean, w))})
    return rec


def torch_part():
    """the yardstick, in a process of its own"""
    import torch

    x, mean, q = table(torch)
    x64, x32 = x.double(), x.float()
    rec = {"moments_f64_ms": timed(torch, lambda: (x64.sum(dim=0), x64.t() @ x64)), "project": []}
    for m in MS:
        w = q[:m].contiguous()
        rec["project"].append({"m": m, "project_f32_ms": timed(torch, lambda: (x32 - mean) @ w.t()),
                               "project_normalised_ms": timed(torch, lambda: torch.nn.functional.normalize((x32 - mean) @ w.t(), dim=1).to(torch.bfloat16))})
    print(json.dumps({"torch": torch.__version__, "form": "f64 x.sum(0), x.T @ x on the widened table (the widening not timed); f32 (x - mean) @ W.T "
                      "on the widened table, then normalize -> bf16", **rec}), flush=True)


def main():
    if "--torch-child" in sys.argv:
        return torch_part()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "projection.json")
    limit = int(sys.argv[sys.argv.index("--torch-timeout") + 1]) if "--torch-timeout" in sys.argv else 300
    record = {"tool": "bench_projection", "warmup": WARM, "runs": RUNS, "engine": engine_part(), "torch_yardstick": "not run yet"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")

    write()  # the engine's figures are on disk before the yardstick starts
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child"], capture_output=True, text=True, timeout=limit)
        if r.returncode == 0:
            record["torch_yardstick"] = json.loads(r.stdout.strip().splitlines()[-1])
        else:
            record["torch_yardstick"] = {"failed": r.returncode, "stderr": r.stderr[-400:]}
    except subprocess.TimeoutExpired:
        record["torch_yardstick"] = {"failed": f"no result within {limit} s"}
    write()
    print(json.dumps(record), flush=True)


if __name__ == "__main__":
    main()
