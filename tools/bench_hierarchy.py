#!/usr/bin/env python3
"""Timing of the cluster hierarchy (K19) on planted data; raw lines go to profiles/hierarchy.txt.

Data: bench_duplicates' -- N / 8 clusters of 8 rows, row = centre + 0.35 * unit noise, L2-normalised bf16 (in-cluster cosines
are >= 0.87, cross-cluster ones <= 0.17 at d = 768); min_samples = 8, so a row's core similarity is its weakest in-cluster
cosine.  N = 4096 and 65 536, d = 768.  Three warm-up runs, seven timed ones; median and range of
  whole      Engine.hierarchy (init + core + the rounds with their read-backs + the sort), device time between two events
  core       Engine.hierarchy_core over all rows (the GEMM and hier_core)
  scan_r / merge_r   round r's Engine.hierarchy_scan over all rows (the GEMM and hier_scan) and Engine.hierarchy_merge
and, in the same process on the same table, the yardstick
  density    Engine.density_clusters (K18: two upper-triangle passes at one threshold, 0.6)
No figure is gated.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_duplicates import RUNS, WARM, planted, stats  # noqa: E402


def main():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    d, min_samples = 768, 8
    for n in (4096, 65536):
        e16 = eng.normalise_rows(planted(torch, n, d))

        def event_ms(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        res = eng.hierarchy(e16, min_samples)
        rounds, components = res["rounds"], res["components"]
        w = res["weights"].cpu().numpy()
        assert components == 1 and len(w) == n - 1
        assert int((w >= 0.6).sum()) == n - n // 8, int((w >= 0.6).sum())  # the planted clusters: 7 tree edges each above the gap
        out = {"tool": "bench_hierarchy", "N": n, "d": d, "min_samples": min_samples, "rounds": rounds, "components": components,
               "warmup": WARM, "runs": RUNS}
        calls = {"whole": lambda: eng.hierarchy(e16, min_samples), "density": lambda: eng.density_clusters(e16, 0.6, min_samples)}
        for name, fn in calls.items():
            for _ in range(WARM):
                fn()
            out[name + "_ms"] = stats([event_ms(fn) for _ in range(RUNS)])
        parts = {"core": []}
        for _ in range(RUNS):
            st = eng.hierarchy_init(n)
            parts["core"].append(event_ms(lambda: eng.hierarchy_core(st, e16, min_samples=min_samples)))
            for r in range(rounds):
                parts.setdefault(f"scan_{r + 1}", []).append(event_ms(lambda: eng.hierarchy_scan(st, e16)))
                parts.setdefault(f"merge_{r + 1}", []).append(event_ms(lambda: eng.hierarchy_merge(st)))
            assert st["counters"].cpu().tolist() == [n - 1, rounds, 1]
        for k, v in parts.items():
            out[k + "_ms"] = stats(v)
        out["whole_over_density"] = out["whole_ms"]["median"] / out["density_ms"]["median"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
