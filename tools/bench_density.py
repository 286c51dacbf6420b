#!/usr/bin/env python3
"""Timing of the density clusters (K18) on planted data; raw lines go to profiles/density.txt.

Data: bench_duplicates' -- N / 8 clusters of 8 rows, row = centre + 0.35 * unit noise, L2-normalised bf16; threshold 0.6
(in-cluster cosines are >= 0.87, cross-cluster ones <= 0.17 at d = 768).  At min_samples = 8 every row has its 7 neighbours
and itself, so every row is core and every pair is a union: the link pass at its most expensive.  N = 4096 and 65 536,
d = 768.  Three warm-up runs, seven timed ones; median and range of
  whole      Engine.density_clusters (init + count + link + finish), device time between two events
  gemm / den_scan / den_finish   the kernel classes of the same call, from the library's event pairs (a profiled run): the
             GEMM of both passes, den_count + den_link, the finish kernels
and, in the same process on the same table, the yardstick
  duplicates Engine.duplicates (K14: one pass over the same blocks)
den_scan's bytes per second are over the f32 values the two passes load (twice bench_duplicates' count).  No figure is gated.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_duplicates import RUNS, WARM, chunks, planted, scan_bytes, stats  # noqa: E402


def main():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    d, tau, min_samples = 768, 0.6, 8
    for n in (4096, 65536):
        e16 = eng.normalise_rows(planted(torch, n, d))

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        res = eng.density_clusters(e16, tau, min_samples)
        summary = res["summary"].cpu().tolist()
        assert summary == [n // 8 * 28, n // 8, n, 0, 0, 8], summary  # the planted clusters: 28 pairs each, all rows core
        assert res["counters"].cpu().tolist() == [summary[0]] * 2
        calls = {"whole": lambda: eng.density_clusters(e16, tau, min_samples), "duplicates": lambda: eng.duplicates(e16, min_sim=tau)}
        out = {"tool": "bench_density", "N": n, "d": d, "min_sim": tau, "min_samples": min_samples, "pairs": summary[0], "clusters": summary[1],
               "chunks_per_pass": len(chunks(n)), "warmup": WARM, "runs": RUNS}
        for name, fn in calls.items():
            for _ in range(WARM):
                fn()
            out[name + "_ms"] = stats([event_ms(fn) for _ in range(RUNS)])
        split = {"cosine": [], "neighbours": [], "cluster": []}
        for _ in range(RUNS):
            eng.profile(True)
            eng.density_clusters(e16, tau, min_samples)
            got = eng.profile_read()
            for k in split:
                split[k].append(got[k][0])
        eng.profile(False)
        out["gemm_ms"], out["den_scan_ms"], out["den_finish_ms"] = stats(split["cosine"]), stats(split["neighbours"]), stats(split["cluster"])
        out["den_scan_bytes"] = 2 * scan_bytes(n)
        out["den_scan_TB_per_s"] = out["den_scan_bytes"] / (out["den_scan_ms"]["median"] * 1e-3) / 1e12
        out["gemm_TFLOP_per_s"] = 2 * sum(2.0 * m * (n - c0) * d for _, m, c0 in chunks(n)) / (out["gemm_ms"]["median"] * 1e-3) / 1e12
        out["whole_over_duplicates"] = out["whole_ms"]["median"] / out["duplicates_ms"]["median"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
