"""Writes tests/golden/silhouette_choose.npz, the fixture of "choosing k" in tests/test_gpu_silhouette.py (no GPU):

    python tests/golden/make_silhouette_case.py [--seeds 40]

silhouette_reference.CHOOSE gives the shape: n rows of d around `centres` planted unit centres, float32 and NOT normalised
(the collection's loader normalises on the GPU).  The data seeds 0 .. are tried in order, and for each the k-means seeds
0 .. 9; the first pair is kept for which, on the rows normalised and rounded to bf16 here, every k of k_range runs with a
score gap above 8 delta(d) (twice what the test asserts, since the GPU's normalisation may round a few elements the other
way) and the best silhouette leads the runner-up by more than 1e-3 (the test asserts 1e-6)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_reference as K  # noqa: E402
import silhouette_reference as S  # noqa: E402


def rows_of(seed):
    c = S.CHOOSE
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((c["centres"], c["d"]))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    truth = rng.integers(0, c["centres"], size=c["n"])
    x = centres[truth] + c["noise"] * rng.standard_normal((c["n"], c["d"])) / np.sqrt(c["d"])
    return (x * rng.uniform(0.5, 2.0, size=(c["n"], 1))).astype(np.float32)


def unit_bits(x32):
    x = x32.astype(np.float64)
    return K.f64_to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


def main():
    seeds = int(sys.argv[sys.argv.index("--seeds") + 1]) if "--seeds" in sys.argv else 40
    c = S.CHOOSE
    for data_seed in range(seeds):
        x32 = rows_of(data_seed)
        bits = unit_bits(x32)
        for seed in range(10):
            runs, picked = S.choose_k(bits, c["k_range"], seed, c["max_iter"])
            gap = min(v["run"]["gap"] for v in runs.values())
            scores = sorted((v["sil"]["score"] for v in runs.values()), reverse=True)
            done = all(v["run"]["converged"] for v in runs.values())
            print(data_seed, seed, "picked", picked, "gap / delta", gap / K.delta(c["d"]), "lead", scores[0] - scores[1], "converged", done, flush=True)
            if done and gap > 8 * K.delta(c["d"]) and scores[0] - scores[1] > 1e-3:
                np.savez(os.path.join(HERE, "silhouette_choose.npz"), x=x32, seed=np.int64(seed), data_seed=np.int64(data_seed), picked=np.int64(picked))
                return 0
    print("no seed found")
    return 1


if __name__ == "__main__":
    sys.exit(main())
