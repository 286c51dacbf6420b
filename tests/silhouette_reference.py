"""Float64 restatement of K16 (include/mme.h, mme_silhouette): the silhouette of a partition of bf16 rows under the distance
d(i, j) = 1 - x_i . x_j, in numpy, for the tests.

Two forms.  `all_pairs` is the textbook one over the N x N matrix (the row's own distance left out of its cluster's sum),
which scikit-learn's silhouette_samples(metric="precomputed") computes on the matrix with a zero diagonal.  `by_sums` is the
library's: the distances from row i to cluster c add up to n_c - x_i . S_c, S_c the sum of the cluster's rows in ascending
row order (kmeans_reference's order), and every formula is evaluated with exactly the operations mme.h writes, in that order
-- so on inputs whose dot products are exact (signed unit basis vectors) the GPU's samples equal these bit for bit, and
elsewhere they differ by the order of the adds inside g = x . S alone."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_reference as K  # noqa: E402

GOLDEN = K.GOLDEN


def cluster_sums(x64, labels, k):
    """(sums f64 [k, d], counts int32 [k]) in ascending row order; a label outside 0..k-1 belongs to no cluster"""
    sums = np.zeros((k, x64.shape[1]))
    counts = np.zeros(k, dtype=np.int32)
    for j in range(k):
        rows = np.nonzero(labels == j)[0]
        counts[j] = len(rows)
        if len(rows):
            sums[j] = np.cumsum(x64[rows], axis=0)[-1]
    return sums, counts


def _finish(sample, labels, k, counts):
    valid = (labels >= 0) & (labels < k)
    cluster = np.full(k, np.nan)
    for j in range(k):
        if counts[j]:
            cluster[j] = np.mean(sample[labels == j])
    used = int((counts > 0).sum())
    rows = int(valid.sum())
    score = float(np.mean(sample[valid])) if used >= 2 and rows > 0 else float("nan")
    return cluster, score, np.array([rows, used], dtype=np.int64)


def by_sums(x_bits, labels, k):
    """The library's form.  -> dict: sample [N] (NaN for a row of no cluster), cluster [k] (NaN when empty), score, info
    [rows counted, clusters with members], sums, counts, a and b (NaN where the formula is not evaluated)."""
    x64 = K.bf16_to_f64(x_bits)
    labels = np.asarray(labels).astype(np.int64)
    n = len(x64)
    sums, counts = cluster_sums(x64, labels, k)
    valid = (labels >= 0) & (labels < k)
    own = np.where(valid, labels, 0)
    G = x64 @ sums.T
    q = np.sum(x64 * x64, axis=1)
    nd = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        M = 1.0 - G / nd[None, :]
        M[:, counts == 0] = np.inf
        M[np.arange(n), own] = np.inf
        b = M.min(axis=1)
        n_own = nd[own]
        g_own = G[np.arange(n), own]
        a = ((n_own - g_own) - (1.0 - q)) / (n_own - 1.0)
        s = (b - a) / np.fmax(a, b)
    s[np.isnan(s)] = 0.0
    s[n_own == 1] = 0.0
    s[~valid] = np.nan
    a[(n_own == 1) | ~valid] = np.nan
    b[~valid] = np.nan
    cluster, score, info = _finish(s, labels, k, counts)
    return {"sample": s, "cluster": cluster, "score": score, "info": info, "sums": sums, "counts": counts, "a": a, "b": b}


def all_pairs(x_bits, labels, k):
    """The textbook form over D = 1 - X X^T; every label must lie in 0..k-1.  -> sample [N]"""
    x64 = K.bf16_to_f64(x_bits)
    labels = np.asarray(labels).astype(np.int64)
    n = len(x64)
    D = 1.0 - x64 @ x64.T
    counts = np.bincount(labels, minlength=k)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), labels] = 1.0
    T = D @ onehot  # the distances from row i to the members of cluster c, its own among them
    s = np.zeros(n)
    for i in range(n):
        c = labels[i]
        if counts[c] <= 1:
            continue
        a = (T[i, c] - D[i, i]) / (counts[c] - 1)
        b = min((T[i, j] / counts[j] for j in range(k) if j != c and counts[j]), default=np.inf)
        v = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
        s[i] = 0.0 if v != v else v
    return s


def sample_bound(ref, d):
    """What separates a GPU sample from by_sums': the f64 dot-product error of g (8 d 2^-53 covers the order of d adds of
    products of magnitude <= n_c, relative to n_c) carried through the final quotient, whose denominator is max(a, b).
    -> (bound, the least max(a, b) over the rows that evaluate the quotient)"""
    with np.errstate(invalid="ignore"):
        m = np.fmax(ref["a"], ref["b"])
    m = m[np.isfinite(m)]
    least = float(m.min()) if len(m) else 1.0
    return 8.0 * d * 2.0 ** -53 / least, least


def planted(n, d, k, seed, noise=0.6, centres=None):
    """bf16 rows around `centres` (default k) planted unit centres and their planted labels (every cluster of 0..centres-1 has
    a member while n >= centres).  -> (x bits [n, d], labels int32 [n])"""
    kt = k if centres is None else centres
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((kt, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    truth = np.concatenate([np.arange(kt), rng.integers(0, kt, size=n - kt)]) if n >= kt else rng.integers(0, kt, size=n)
    truth = truth[rng.permutation(n)]
    x = c[truth] + noise * rng.standard_normal((n, d)) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return K.f64_to_bf16(x), truth.astype(np.int32)


# ---- choosing k: the fixture of tests/test_gpu_silhouette.py (tests/golden/make_silhouette_case.py searches its seed) ----

CHOOSE = {"n": 512, "d": 64, "centres": 4, "noise": 0.9, "k_range": range(2, 9), "max_iter": 100}


def pick(scores):
    """region_compare.pick_n_clusters restated: ascending k, strict >, from -1, NaN skipped"""
    ks = sorted(scores)
    best, best_k = -1, ks[0]
    for k in ks:
        v = scores[k]
        if v is None or v != v:
            continue
        if v > best:
            best, best_k = v, k
    return best_k


def choose_k(x_bits, k_range, seed, max_iter):
    """kmeans_regions(n_clusters=None, init="random", n_init=1) restated: per k the start rows numpy's default_rng(seed) draws
    (region_compare.kmeans_init_rows), K15's float64 run, the silhouette of its labels.  -> {k: {"run", "sil"}}, picked k"""
    n = len(x_bits)
    out = {}
    for k in sorted(int(k) for k in k_range if 2 <= int(k) <= n):
        rows = np.sort(np.random.default_rng(int(seed)).choice(n, size=k, replace=False)).astype(np.int32)
        run = K.run(x_bits, x_bits[rows], max_iter)
        out[k] = {"run": run, "sil": by_sums(x_bits, run["labels"], k), "rows": rows}
    return out, pick({k: v["sil"]["score"] for k, v in out.items()})
