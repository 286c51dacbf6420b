#!/usr/bin/env python3
"""Timing of the near-duplicate groups (K14) on planted data; raw lines go to profiles/duplicates.txt.

Data: N / 8 clusters of 8 rows, row = centre + 0.35 * unit noise, L2-normalised bf16; threshold 0.6 (in-cluster cosines are
>= 0.87, cross-cluster ones <= 0.17 at d = 768, so the graph is exactly the planted clusters).  N = 4096 and 65 536, d = 768.
Three warm-up runs, seven timed ones; median and range of
  whole      Engine.duplicates (init + scan + finish), device time between two events
  gemm / dup_scan / dup_finish   the kernel classes of the same call, from the library's event pairs (a profiled run)
and, in the same process on the same table, the yardsticks
  neighbours Engine.neighbours over all rows (K12, fetch 30, top 10)
  cosine     Engine.cosine of the first chunk's rows against all rows (K9: the block one chunk writes)
dup_scan's bytes per second are over the f32 values it loads: per row, the 1024-value segments from the one that holds the
diagonal on.  No figure is gated.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WARM, RUNS, SEG = 3, 7, 1024


def planted(torch, n, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(n // 8, d, generator=g, device="cuda"), dim=1)
    noise = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    return centres.repeat_interleave(8, dim=0) + 0.35 * noise


def chunks(n, ws_bytes=2048 << 20):
    """the host pass's chunks (capi_duplicates.hip): (first row, rows, first column)"""
    out, q = [], 0
    while q < n:
        c0 = q & ~3
        ld = (n - c0 + 3) & ~3
        rc = max(256, ws_bytes // (ld * 4) // 256 * 256)
        m = min(n - q, rc)
        out.append((q, m, c0))
        q += m
    return out


def scan_bytes(n):
    total = 0
    for q, m, c0 in chunks(n):
        first = np.arange(q, q + m, dtype=np.int64) - c0 + 1
        total += int(((n - c0) - first // SEG * SEG).clip(min=0).sum()) * 4
    return total


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    d, tau = 768, 0.6
    for n in (4096, 65536):
        e16 = eng.normalise_rows(planted(torch, n, d))
        rows0 = chunks(n)[0][1]

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        res = eng.duplicates(e16, min_sim=tau)
        summary = res["summary"].cpu().tolist()
        assert summary == [n // 8 * 28, n // 8, n, 8], summary  # the planted clusters, 28 edges each
        calls = {"whole": lambda: eng.duplicates(e16, min_sim=tau), "neighbours": lambda: eng.neighbours(e16, fetch=30, top_n=10),
                 "cosine": lambda: eng.cosine(e16[:rows0], e16)}
        out = {"tool": "bench_duplicates", "N": n, "d": d, "min_sim": tau, "edges": summary[0], "chunks": len(chunks(n)), "first_chunk_rows": rows0,
               "warmup": WARM, "runs": RUNS}
        for name, fn in calls.items():
            for _ in range(WARM):
                fn()
            out[name + "_ms"] = stats([event_ms(fn) for _ in range(RUNS)])
        split = {"cosine": [], "neighbours": [], "cluster": []}
        for _ in range(RUNS):
            eng.profile(True)
            eng.duplicates(e16, min_sim=tau)
            got = eng.profile_read()
            for k in split:
                split[k].append(got[k][0])
        eng.profile(False)
        out["gemm_ms"], out["dup_scan_ms"], out["dup_finish_ms"] = stats(split["cosine"]), stats(split["neighbours"]), stats(split["cluster"])
        out["dup_scan_bytes"] = scan_bytes(n)
        out["dup_scan_TB_per_s"] = out["dup_scan_bytes"] / (out["dup_scan_ms"]["median"] * 1e-3) / 1e12
        out["gemm_TFLOP_per_s"] = sum(2.0 * m * (n - c0) * d for _, m, c0 in chunks(n)) / (out["gemm_ms"]["median"] * 1e-3) / 1e12
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
