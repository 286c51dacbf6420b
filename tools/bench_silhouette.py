#!/usr/bin/env python3
"""Timing of the silhouette over the vector table (K16) on seeded synthetic rows; the record goes to
profiles/silhouette.json.

    python tools/bench_silhouette.py [--out profiles/silhouette.json] [--step-timeout 300]

Data: N = 65 536 rows of d = 768 around k planted unit centres (tools/bench_kmeans.py's table), for k = 2, 10, 64 and 1024; the
labels scored are the planted ones.  Three warm-up runs, seven timed ones, median and range, from HIP events:
  rows     silhouette_rows alone (mme_silhouette_rows on the sums and counts of the whole call)
  whole    mme_silhouette: K15's update on the labels, silhouette_rows, the two reductions
  kmeans   one mme_kmeans run at the same k from k seeded start rows, max_iter = 100, with the iterations it ran
  choose   what region_compare does for n_clusters = None over k = 2..10 on one table (6 planted centres): per k one
           mme_kmeans run and one mme_silhouette of its labels; the ratio is (runs + silhouettes) / runs
The rows kernel's rate counts 2 N d k flop against the 78.6 TFLOP/s f64 peak of the MI355X.
This process never opens the GPU.  The engine's figures come from a child under `timeout -k 10` and are written first; only
then the torch yardstick (x.double() @ sums.T and the elementwise tail, per k) runs in a child of its own under its own
timeout and is merged in when it comes back; if either does not, the record says so.  scikit-learn's silhouette_score(metric=
"cosine") at N = 8192, k = 10 is timed on the host last.  No figure is gated.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, RUNS = 3, 7
N, D, KS = 65536, 768, (2, 10, 64, 1024)
CHOOSE_KS, CHOOSE_CENTRES = tuple(range(2, 11)), 6
PEAK_F64 = 78.6e12
HOST_N, HOST_K = 8192, 10


def table(torch, k, seed=0, n=N, device="cuda"):
    """bf16 [n, D] unit rows around k planted centres, the planted labels and k start rows (seeded; bench_kmeans' table)"""
    g = torch.Generator(device=device).manual_seed(seed + k)
    centres = torch.nn.functional.normalize(torch.randn(k, D, generator=g, device=device), dim=1)
    noise = torch.nn.functional.normalize(torch.randn(n, D, generator=g, device=device), dim=1)
    which = torch.randint(0, k, (n,), generator=g, device=device)
    x = torch.nn.functional.normalize(centres[which] + 0.8 * noise, dim=1).to(torch.bfloat16)
    rows = torch.randperm(n, generator=g, device=device)[:k].sort().values
    return x, which.to(torch.int32), rows


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
    return stats([event_ms(torch, fn) for _ in range(RUNS)])


def engine_part():
    import torch

    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    shapes = []
    for k in KS:
        x, labels, rows = table(torch, k)
        res = eng.silhouette(x, labels, k, samples=True)
        sample = torch.empty(N, dtype=torch.float64, device="cuda")
        rec = {"N": N, "d": D, "k": k, "score": float(res.score.item()), "clusters_with_members": int(res.info[1].item())}
        rec["rows_ms"] = timed(torch, lambda: eng.silhouette_rows(x, labels, res.sums, res.counts, sample))
        assert torch.equal(sample, res.samples)
        rec["whole_ms"] = timed(torch, lambda: eng.silhouette(x, labels, k))
        rec["rows_tflops"] = 2.0 * N * D * k / (rec["rows_ms"]["median"] * 1e-3) / 1e12
        rec["rows_fraction_of_f64_peak"] = rec["rows_tflops"] * 1e12 / PEAK_F64
        start = rows.cpu().numpy()
        last = [None]

        def run():
            last[0] = eng.kmeans(x, k, init_rows=start, max_iter=100)

        rec["kmeans_ms"] = timed(torch, run)
        rec["kmeans_iterations"] = int(last[0].info[0].item())
        shapes.append(rec)
    x, _, _ = table(torch, CHOOSE_CENTRES, seed=100)
    choose = {"planted_centres": CHOOSE_CENTRES, "per_k": []}
    for k in CHOOSE_KS:
        start = torch.randperm(N, generator=torch.Generator(device="cuda").manual_seed(k), device="cuda")[:k].sort().values.cpu().numpy()
        last = [None]

        def run():
            last[0] = eng.kmeans(x, k, init_rows=start, max_iter=100)

        km = timed(torch, run)
        labels = last[0].labels
        sil = timed(torch, lambda: eng.silhouette(x, labels, k))
        choose["per_k"].append({"k": k, "kmeans_ms": km, "kmeans_iterations": int(last[0].info[0].item()), "silhouette_ms": sil,
                                "score": float(eng.silhouette(x, labels, k).score.item())})
    runs = sum(r["kmeans_ms"]["median"] for r in choose["per_k"])
    sils = sum(r["silhouette_ms"]["median"] for r in choose["per_k"])
    choose.update({"kmeans_runs_ms": runs, "silhouettes_ms": sils, "ratio_choose_to_runs_alone": (runs + sils) / runs})
    return {"shapes": shapes, "choose_k_2_to_10": choose}


def torch_part():
    """the yardstick, in a process of its own: plain torch for the product and the tail (the sums by index_add_ are not timed)"""
    import torch

    out = []
    for k in KS:
        x, labels, _ = table(torch, k)
        lab = labels.long()
        x64 = x.double()
        sums = torch.zeros((k, D), dtype=torch.float64, device="cuda").index_add_(0, lab, x64)
        n = torch.bincount(lab, minlength=k).double()
        ar = torch.arange(N, device="cuda")

        def score():
            g = x.double() @ sums.T
            q = (x.double() ** 2).sum(1)
            own, n_own = g[ar, lab], n[lab]
            a = ((n_own - own) - (1.0 - q)) / (n_own - 1.0)
            m = 1.0 - g / n
            m[:, n == 0] = float("inf")
            m[ar, lab] = float("inf")
            b = m.min(dim=1).values
            s = torch.nan_to_num((b - a) / torch.maximum(a, b), nan=0.0)
            s[n_own == 1] = 0.0
            return s.mean()

        rec = {"k": k, "score_ms": timed(torch, score), "score": float(score().item())}
        out.append(rec)
    print(json.dumps({"torch": torch.__version__, "form": "x.double() @ sums.T -> gather, 1 - g / n, masked min, quotient, mean", "shapes": out}), flush=True)


def host_part():
    """scikit-learn on the host, no device: the CPU figure only"""
    import torch
    from sklearn.metrics import silhouette_score

    x, labels, _ = table(torch, HOST_K, n=HOST_N, device="cpu")
    x64 = x.double().numpy()
    t0 = time.perf_counter()
    score = float(silhouette_score(x64, labels.numpy(), metric="cosine"))
    return {"N": HOST_N, "d": D, "k": HOST_K, "seconds": time.perf_counter() - t0, "score": score}


def child(flag, limit):
    """this tool again with `flag`, under timeout -k 10: the last line of its output as JSON, or what went wrong"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), flag], capture_output=True, text=True)
    if r.returncode != 0:
        return None, {"failed": r.returncode, "stderr": r.stderr[-400:]}
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
    if "--engine-child" in sys.argv:
        print(json.dumps(engine_part()), flush=True)
        return 0
    if "--torch-child" in sys.argv:
        torch_part()
        return 0
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "silhouette.json")
    limit = int(sys.argv[sys.argv.index("--step-timeout") + 1]) if "--step-timeout" in sys.argv else 300
    record = {"tool": "bench_silhouette", "warmup": WARM, "runs": RUNS, "f64_peak_tflops": PEAK_F64 / 1e12, "engine": "not run yet",
              "torch_yardstick": "not run yet", "sklearn_host": "not run yet"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")

    got, err = child("--engine-child", limit)
    record["engine"] = got if err is None else err
    write()  # the engine's figures are on disk before the yardstick starts
    if err is not None:  # nothing more is started on the GPU after a step that failed
        record["torch_yardstick"] = "not run: the engine step failed"
        write()
        print(json.dumps(record), flush=True)
        return 1
    got, err = child("--torch-child", limit)
    record["torch_yardstick"] = got if err is None else err
    write()
    if err is None:
        record["sklearn_host"] = host_part()
        write()
    print(json.dumps(record), flush=True)
    return 0 if err is None else 1


if __name__ == "__main__":
    sys.exit(main())
