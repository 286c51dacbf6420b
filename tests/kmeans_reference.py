"""Float64 restatement of K15 (include/mme.h, mme_kmeans): spherical k-means over bf16 rows, in numpy, for the tests.

The sequence is the library's: assign against the start; then up to max_iter iterations of { update; assign; step end },
stopped after the first iteration that moved no row (that iteration is counted).  Scores are float64 dot products of the
bf16 rows; the argmax takes the lowest index; the sums run in ascending row order in float64 (np.cumsum is sequential);
a centroid is sums / max(sqrt(sum of squares in ascending column order), 1e-12), rounded ONCE from float64 to bf16, nearest
even.  An empty cluster keeps its centroid.  Every assignment records the gap between each row's best and second-best
score; `gap` is the smallest over the whole run -- the GPU's f32-accumulated scores are within delta(d) of these, so a run
with gap > 2 delta makes the same decisions (the tests ask 4 delta)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def delta(d):
    """K14's bound (mme.h) for an f32-accumulated dot of bf16 unit rows against float64"""
    return 2.0 * d * 2.0 ** -24


def bf16_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f64_to_bf16(x):
    """float64 -> bf16 bits, ONE rounding, nearest even.  Picks among the three bf16 neighbours of the f32 image by their
    exact float64 distance to x (the differences of such close numbers are exact), ties to the even pattern."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError("finite values only")
    mag = np.abs(x)
    b = (mag.astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
    cands = np.stack([np.maximum(b - 1, 0), b, b + 1])
    vals = (cands.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    err = np.abs(vals - mag)
    best = err.min(axis=0)
    ok = err == best
    even = ok & (cands % 2 == 0)
    pick = np.where(even.any(axis=0), np.argmax(even, axis=0), np.argmax(ok, axis=0))
    out = np.take_along_axis(cands, pick[None], axis=0)[0].astype(np.uint16)
    return out | (np.signbit(x).astype(np.uint16) << 15)


def scores(x64, c64):
    return x64 @ c64.T


def assign(x64, c64, cen_bits=None):
    """(labels, score of the label, smallest best-minus-second gap).  With cen_bits, centroids that are bit-identical to the
    winner do not count as a second best: their scores are the winner's on any implementation that treats every column
    alike, and the lowest index wins (the case of a start that lists two equal rows)."""
    S = scores(x64, c64)
    lab = np.argmax(S, axis=1)  # the first of equal maxima
    best = S[np.arange(len(S)), lab]
    T = S.copy()
    T[np.arange(len(S)), lab] = -np.inf
    if cen_bits is not None:
        _, cls = np.unique(np.asarray(cen_bits), axis=0, return_inverse=True)
        cls = cls.reshape(-1)
        T[cls[None, :] == cls[lab][:, None]] = -np.inf
    return lab.astype(np.int32), best, float((best - T.max(axis=1)).min())


def update(x64, labels, cen_bits):
    """(sums f64 [k, d], counts int32 [k], new centroid bits) from the labels; labels outside 0..k-1 belong to no cluster"""
    k, d = cen_bits.shape
    sums = np.zeros((k, d))
    counts = np.zeros(k, dtype=np.int32)
    out = cen_bits.copy()
    for j in range(k):
        rows = np.nonzero(labels == j)[0]  # ascending
        counts[j] = len(rows)
        if len(rows) == 0:
            continue
        s = np.cumsum(x64[rows], axis=0)[-1]
        sums[j] = s
        n2 = np.cumsum(s * s)[-1]
        out[j] = f64_to_bf16(s / max(np.sqrt(n2), 1e-12))
    return sums, counts, out


def run(x_bits, start_bits, max_iter):
    x64 = bf16_to_f64(x_bits)
    cen = np.array(start_bits, dtype=np.uint16)
    k, d = cen.shape
    labels, sim, gap = assign(x64, bf16_to_f64(cen), cen)
    sums, counts = np.zeros((k, d)), np.zeros(k, dtype=np.int32)
    iterations = moved = empty = 0
    converged = False
    for _ in range(max_iter):
        sums, counts, cen = update(x64, labels, cen)
        new, sim, g = assign(x64, bf16_to_f64(cen), cen)
        gap = min(gap, g)
        moved = int((new != labels).sum())
        labels = new
        iterations += 1
        empty = int((counts == 0).sum())
        if moved == 0:
            converged = True
            break
    return {"labels": labels, "sim": sim, "centroids": cen, "sums": sums, "counts": counts, "iterations": iterations, "moved": moved,
            "converged": converged, "empty": empty, "gap": gap, "objective": float(sim.sum())}


def blobs(n, d, kt, k, noise, seed):
    """The generator of the whole-run fixtures (tests/golden/make_kmeans_cases.py): kt random unit centres, rows = centre +
    noise N(0, 1) / sqrt(d), normalised, rounded to bf16; start = sorted choice(n, k).  -> (x bits, start rows int32, truth)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((kt, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    truth = rng.integers(0, kt, size=n)
    x = c[truth] + noise * rng.standard_normal((n, d)) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    rows = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
    return f64_to_bf16(x), rows, truth.astype(np.int32)


# name -> (n, d, kt, k, noise): the seeds were searched on the CPU (make_kmeans_cases.py) for a run of several iterations
# whose gap exceeds 4 delta(d); the wide tables get fewer rows, as the narrow margin of d * 2^-23 demands
CASES = {
    "d64": (300, 64, 5, 7, 1.0),
    "d128": (300, 128, 5, 7, 1.0),
    "d384": (517, 384, 6, 9, 1.2),
    "d768": (150, 768, 3, 4, 1.0),
    "d1024": (120, 1024, 3, 4, 1.0),
}


def load_case(name):
    """(x bits uint16 [n, d], start rows int32 [k]) of a committed fixture"""
    g = np.load(os.path.join(GOLDEN, f"kmeans_{name}.npz"))
    return g["x"], g["rows"]
