"""Writes tests/golden/kmeans_<name>.npz, the whole-run fixtures of tests/test_gpu_kmeans.py (no GPU):

    python tests/golden/make_kmeans_cases.py [--seeds 40]

For each shape of kmeans_reference.CASES the seeds 0 .. are tried in order; the first whose float64 run takes at least
MIN_ITER iterations, converges, and keeps every row's best score more than 4 delta(d) above its second best is written
(x: the bf16 rows as uint16, rows: the start rows, seed, and the reference's iterations and gap for the record)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_reference as R  # noqa: E402

MIN_ITER = {"d64": 4, "d128": 4, "d384": 3, "d768": 2, "d1024": 2}


def search(name, seeds):
    n, d, kt, k, noise = R.CASES[name]
    found = 0
    for seed in range(seeds):
        x, rows, _ = R.blobs(n, d, kt, k, noise, seed)
        ref = R.run(x, x[rows], 50)
        ok = ref["converged"] and ref["iterations"] >= MIN_ITER[name] and ref["gap"] > 4 * R.delta(d)
        found += ok
        if ok and found == 1:
            best = (seed, x, rows, ref)
    print(f"{name}: {found} of {seeds} seeds qualify", end="")
    if not found:
        print()
        return False
    seed, x, rows, ref = best
    print(f"; seed {seed}: {ref['iterations']} iterations, gap {ref['gap']:.3g} = {ref['gap'] / R.delta(d):.1f} delta")
    np.savez(os.path.join(HERE, f"kmeans_{name}.npz"), x=x, rows=rows, seed=np.int64(seed), iterations=np.int64(ref["iterations"]),
             gap=np.float64(ref["gap"]))
    return True


if __name__ == "__main__":
    seeds = int(sys.argv[sys.argv.index("--seeds") + 1]) if "--seeds" in sys.argv else 40
    sys.exit(0 if all([search(name, seeds) for name in R.CASES]) else 1)
