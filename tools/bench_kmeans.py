#!/usr/bin/env python3
"""Timing of spherical k-means (K15) on seeded synthetic rows; the record goes to profiles/kmeans.json.

    python tools/bench_kmeans.py [--out profiles/kmeans.json] [--torch-timeout 300]

Data: N = 65 536 rows of d = 768 around k planted unit centres (row = centre + 0.8 unit noise, L2-normalised bf16), for
k = 64 and k = 1024; the centroids are k seeded rows of the table.  Three warm-up runs, seven timed ones, median and range, all
from HIP events:
  assign   one mme_kmeans_apply ASSIGN over all rows, split by the library's event pairs into its GEMM ("cosine") and
           kmeans_argmax_rows ("cluster")
  update   one mme_kmeans_apply UPDATE from those labels (the counting sort, the f64 sums, the centroids)
  cosine   Engine.cosine for the same [N, k] block, in the same process on the same table: what an iteration costs beyond its
           GEMM is assign + update - cosine
  whole    mme_kmeans from that start, max_iter = 20, between two events, with the iterations it ran
The engine's figures are written first.  The torch yardstick (bf16 mm -> argmax -> f32 index_add_ -> normalise, per iteration)
then runs in a fresh child process under its own timeout and is merged into the record when it comes back; if it does not,
the record says so and keeps the engine's figures.  No figure is gated.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, RUNS = 3, 7
N, D, KS = 65536, 768, (64, 1024)


def table(torch, k, seed=0):
    """bf16 [N, D] unit rows around k planted centres, and the k start rows (seeded)"""
    g = torch.Generator(device="cuda").manual_seed(seed + k)
    centres = torch.nn.functional.normalize(torch.randn(k, D, generator=g, device="cuda"), dim=1)
    noise = torch.nn.functional.normalize(torch.randn(N, D, generator=g, device="cuda"), dim=1)
    which = torch.randint(0, k, (N,), generator=g, device="cuda")
    x = torch.nn.functional.normalize(centres[which] + 0.8 * noise, dim=1).to(torch.bfloat16)
    rows = torch.randperm(N, generator=g, device="cuda")[:k].sort().values
    return x, rows


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


def engine_part():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    out = []
    for k in KS:
        x, rows = table(torch, k)
        cen = x[rows].contiguous()
        labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        sim = torch.empty(N, dtype=torch.float32, device="cuda")
        moved = torch.zeros(1, dtype=torch.int64, device="cuda")
        sums = torch.empty((k, D), dtype=torch.float64, device="cuda")
        counts = torch.empty(k, dtype=torch.int32, device="cuda")
        new_cen = cen.clone()
        block = torch.empty((N, k), dtype=torch.float32, device="cuda")
        assign = lambda: eng.kmeans_apply("assign", emb=x, centroids=cen, labels=labels, sim=sim, moved=moved)  # noqa: E731
        update = lambda: eng.kmeans_apply("update", emb=x, labels=labels, centroids=new_cen, sums=sums, counts=counts)  # noqa: E731
        cosine = lambda: eng.cosine(x, cen, out=block)  # noqa: E731
        rec = {"N": N, "d": D, "k": k}
        assign()
        rec["cluster_sizes"] = {"min": int(torch.bincount(labels.long(), minlength=k).min()), "max": int(torch.bincount(labels.long(), minlength=k).max())}
        split = {"assign_gemm_ms": [], "assign_argmax_ms": [], "update_ms": []}
        for it in range(WARM + RUNS):
            eng.profile(True)
            assign()
            got = eng.profile_read()
            eng.profile(True)
            update()
            upd = eng.profile_read()
            if it >= WARM:
                split["assign_gemm_ms"].append(got["cosine"][0])
                split["assign_argmax_ms"].append(got["cluster"][0])
                split["update_ms"].append(upd["cluster"][0])
        eng.profile(False)
        for name, v in split.items():
            rec[name] = stats(v)
        rec["assign_ms"] = stats([a + b for a, b in zip(split["assign_gemm_ms"], split["assign_argmax_ms"])])
        for _ in range(WARM):
            cosine()
        rec["cosine_ms"] = stats([event_ms(torch, cosine) for _ in range(RUNS)])
        rec["iteration_beyond_gemm_ms"] = rec["assign_ms"]["median"] + rec["update_ms"]["median"] - rec["cosine_ms"]["median"]
        whole = lambda: eng.kmeans(x, k, init_rows=rows.cpu().numpy(), max_iter=20)  # noqa: E731
        for _ in range(WARM):
            res = whole()
        rec["whole_max_iter_20_ms"] = stats([event_ms(torch, whole) for _ in range(RUNS)])
        rec["whole_iterations"], rec["whole_converged"] = int(res.info[0].item()), bool(res.info[2].item())
        out.append(rec)
    return out


def torch_part():
    """the yardstick, in a process of its own: plain torch for one iteration's two halves"""
    import torch

    out = []
    for k in KS:
        x, rows = table(torch, k)
        cen = x[rows].contiguous()
        x32 = x.float()
        labels = [None]

        def assign():
            labels[0] = torch.mm(x, cen.t()).argmax(dim=1)

        def update():
            s = torch.zeros((k, D), dtype=torch.float32, device="cuda").index_add_(0, labels[0], x32)
            return torch.nn.functional.normalize(s, dim=1).to(torch.bfloat16)

        rec = {"k": k}
        for name, fn in (("assign_ms", assign), ("update_ms", update)):
            for _ in range(WARM):
                fn()
            rec[name] = stats([event_ms(torch, fn) for _ in range(RUNS)])
        out.append(rec)
    print(json.dumps({"torch": torch.__version__, "form": "bf16 mm -> argmax; zeros -> f32 index_add_ -> normalize -> bf16", "shapes": out}), flush=True)


def main():
    if "--torch-child" in sys.argv:
        return torch_part()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kmeans.json")
    limit = int(sys.argv[sys.argv.index("--torch-timeout") + 1]) if "--torch-timeout" in sys.argv else 300
    record = {"tool": "bench_kmeans", "warmup": WARM, "runs": RUNS, "engine": engine_part(), "torch_yardstick": "not run yet"}

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
