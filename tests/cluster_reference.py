"""float64 reference of the page clustering (K11) that is fast enough for thousands of pages, and the seeded inputs its
tests share.

Written from the published algorithms -- scipy's `linkage(..., 'average')` (nearest-neighbour chain over a distance
matrix, stable sort of the merges by height, union-find relabel), scikit-learn's `_hc_cut` and `silhouette_score`, and
the k selection of weighted_region_clustering.py:482-490 -- with each scan one numpy operation over a full symmetric
matrix, so that a tree of 4096 pages takes a second where oracle/cluster.py's literal loops take hours.  The tie rules
are the ones that decide labels: a scan takes the FIRST minimum of the live row (`argmin`), and the previous chain
element wins unless a scanned distance is strictly smaller.  `linkage_average` takes those rules as switches so that a
test can state a plausible kernel bug as a change of the reference (see MUTANTS).

The generators below rebuild every case of tests/golden/cluster_scale_cases.npz from its seed; the golden file stores
only a hash of each matrix, labels and silhouettes (tests/golden/make_cluster_scale_golden.py).
"""
import functools
import hashlib

import numpy as np

from oracle.cluster import hc_cut, silhouette_precomputed

MODES = ("reference_fallback", "precomputed")

# the changes of the reference that the tie cases must separate: name -> keyword arguments of linkage_average
MUTANTS = {
    "highest_index_wins": {"tie": "high"},
    "previous_not_preferred": {"prefer_prev": False},
    "unstable_height_sort": {"stable": False},
    "scan_stops_at_1024": {"scan_limit": 1024},
}


def linkage_average(Y, *, tie="low", prefer_prev=True, stable=True, scan_limit=None):
    """scipy `linkage(squareform(Y), 'average')` on the full symmetric distance matrix Y [n, n].

    Returns (children int64 [n-1, 2], heights f64 [n-1]): the merges sorted by height (stable) and relabelled to scipy's
    node numbering, lower id first.  The keyword arguments are mutants: tie="high" takes the last minimum of a scan,
    prefer_prev=False lets a scanned distance equal to the previous chain element's replace it, stable=False reverses
    the order among equal heights, scan_limit=L leaves indices >= L out of every nearest-neighbour scan."""
    D = np.array(Y, dtype=np.float64)
    n = D.shape[0]
    size = np.ones(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    row = np.empty(n, dtype=np.float64)
    Zx = np.empty(n - 1, dtype=np.int64)
    Zy = np.empty(n - 1, dtype=np.int64)
    Zh = np.empty(n - 1, dtype=np.float64)
    chain = []
    for k in range(n - 1):
        if not chain:
            chain.append(int(np.argmax(live)))  # first live cluster
        while True:
            x = chain[-1]
            np.copyto(row, D[x])
            row[~live] = np.inf
            row[x] = np.inf
            if scan_limit is not None and np.isfinite(row[:scan_limit]).any():
                row[scan_limit:] = np.inf  # (an empty scan would leave the mutant without any neighbour: it scans all then)
            y = int(np.argmin(row)) if tie == "low" else n - 1 - int(np.argmin(row[::-1]))
            cur = row[y]
            if len(chain) > 1:
                prev = chain[-2]
                dprev = D[x, prev]
                keep_prev = not (cur < dprev) if prefer_prev else not (cur <= dprev)
                if keep_prev or len(chain) == n:  # (the second only bounds a mutant's chain)
                    y, cur = prev, dprev
                if y == prev:
                    break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        Zx[k], Zy[k], Zh[k] = x, y, cur
        size[x], size[y] = 0, nx + ny
        live[x] = False
        new = (nx * D[x] + ny * D[y]) / (nx + ny)  # Lance-Williams, average: (n_x d_xi + n_y d_yi) / (n_x + n_y)
        new[y] = D[y, y]
        D[y, :] = new
        D[:, y] = new
    order = np.argsort(Zh, kind="stable") if stable else np.lexsort((-np.arange(n - 1), Zh))
    # scipy's `label`: union-find over the merges in height order
    parent = list(range(2 * n - 1))
    children = np.empty((n - 1, 2), dtype=np.int64)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for r, k in enumerate(order):
        a, b = find(int(Zx[k])), find(int(Zy[k]))
        children[r] = (a, b) if a < b else (b, a)
        parent[a] = parent[b] = n + r
    return children, Zh[order]


def cut(children, k):
    """labels int64 [n] of the tree cut into k clusters (scikit-learn `_hc_cut`)"""
    return hc_cut(int(k), children, len(children) + 1)


def silhouette(D, labels):
    """scikit-learn silhouette_score(D, labels, metric='precomputed')"""
    return silhouette_precomputed(D, labels)


def pdist_rows(D):
    """Full matrix of euclidean distances between the rows of D, each sum of squares accumulated column by column in
    f64 (scipy pdist 'euclidean')."""
    D = np.asarray(D, dtype=np.float64)
    n, m = D.shape
    DT = np.ascontiguousarray(D.T)
    s = np.zeros((n, n), dtype=np.float64)
    t = np.empty((n, n), dtype=np.float64)
    for k in range(m):
        col = DT[k]
        np.subtract(col[:, None], col[None, :], out=t)
        np.multiply(t, t, out=t)
        s += t
    return np.sqrt(s, out=s)


def tree(S, mode, **mutant):
    """(D, children, heights) of the similarity matrix S with its diagonal taken as 1"""
    S = np.array(S, dtype=np.float64)
    np.fill_diagonal(S, 1.0)
    D = 1.0 - S
    Y = pdist_rows(D) if mode == "reference_fallback" else D
    children, heights = linkage_average(Y, **mutant)
    return D, children, heights


def max_auto_k(S):
    """weighted_region_clustering.py:482-490: the largest k the silhouette search tries"""
    P = S.shape[0]
    nonzero_pairs = int(np.sum(S > 0.01)) - P
    return min(3, P) if nonzero_pairs < 10 else min(10, P)


def cluster(S, n_clusters=None, mode="reference_fallback", **mutant):
    """What `cluster_images` computes, for any number of cuts of one tree.

    n_clusters: None, an int or a sequence of ints.  Returns a dict: "labels" {k: int64 [P]} for each requested k,
    "scores" [(k, silhouette)] for k = 2..max k where scikit-learn defines it (1 < k < P), "auto_k" and "auto_labels"
    (strict `>` argmax starting from -1 with k = 2), "children" and "heights" of the tree."""
    S = np.array(S, dtype=np.float64)
    np.fill_diagonal(S, 1.0)
    D, children, heights = tree(S, mode, **mutant)
    P = S.shape[0]
    ks = [] if n_clusters is None else ([int(n_clusters)] if np.isscalar(n_clusters) else [int(k) for k in n_clusters])
    out = {"labels": {k: cut(children, k) for k in ks}, "children": children, "heights": heights, "scores": []}
    best_score, best_k = -1, 2
    for k in range(2, max_auto_k(S) + 1):
        if not k < P:
            continue
        score = silhouette(D, cut(children, k))
        out["scores"].append((k, score))
        if score > best_score:
            best_score, best_k = score, k
    out["auto_k"] = best_k
    out["auto_labels"] = cut(children, best_k)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs


def blocked(P, seed):
    """The blocked random family of test_gpu_cluster.test_large_seeded_matrices_vs_oracle: seven groups of pages, a
    fifth of the entries zero, largest off-diagonal entry 1."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 7, P)
    A = rng.random((P, P)) * 0.3 + 0.6 * (g[:, None] == g[None, :]) * rng.random((P, P))
    S = (A + A.T) / 2
    S[rng.random((P, P)) < 0.2] = 0.0
    S = np.minimum(S, S.T)
    S /= np.max(S - np.diag(np.diag(S)))
    np.fill_diagonal(S, 1.0)
    return S


def planted_ties(P, seed):
    """Entries from {0, 1/4, 1/2, 3/4}, symmetric; about one page in ten is an exact copy of another (same row and
    column, similarity 1 between the two)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (P, P)) / 4.0
    S = np.triu(A, 1)
    S = S + S.T
    src = np.arange(P)
    for i in range(1, P):
        if rng.random() < 0.1:
            src[i] = src[rng.integers(0, i)]  # a copy of an original page (never of a copy)
    S = S[np.ix_(src, src)]
    S[src[:, None] == src[None, :]] = 1.0
    np.fill_diagonal(S, 1.0)
    return S


def singletons(P, seed, outliers=5):
    """blocked(P), with `outliers` pages whose similarity to every other page is 0"""
    S = blocked(P, seed)
    out = np.random.default_rng(seed + 1000).choice(P, outliers, replace=False)
    S[out, :] = 0.0
    S[:, out] = 0.0
    np.fill_diagonal(S, 1.0)
    return S


def _depth(P):
    return (1, 11, 64, P - 1, P)


BASE_KS = (2, 3, 10)

# name -> (generator, arguments, modes with a golden, fixed n_clusters listed in the golden: see listed_ks)
CASES = {
    "blocked1025": (blocked, (1025, 11), MODES, BASE_KS + _depth(1025)),
    "blocked1100": (blocked, (1100, 12), MODES, BASE_KS),
    "blocked2049": (blocked, (2049, 13), MODES, BASE_KS),
    "blocked4096": (blocked, (4096, 14), MODES, BASE_KS + (11, 1000, 4095, 4096)),
    "ties96": (planted_ties, (96, 21), MODES, BASE_KS + (5, 7)),
    "ties1030": (planted_ties, (1030, 22), MODES, BASE_KS + (5, 7)),
    "eye5": (np.eye, (5,), MODES, (2, 3)),
    "eye1500": (np.eye, (1500,), MODES, BASE_KS),
    "singletons130": (singletons, (130, 31), MODES, BASE_KS + (5, 6, 7) + _depth(130)),
}
TIE_CASES = ("ties96", "ties1030", "eye5", "eye1500")
# a fallback-mode call at 4096 pages takes most of a second on the GPU (the row-distance pass): fewer of them
FALLBACK_KS = {"blocked4096": (10,)}


def listed_ks(name, mode):
    """the fixed n_clusters whose labels the golden holds for this case and mode"""
    if mode == "reference_fallback" and name in FALLBACK_KS:
        return FALLBACK_KS[name]
    return CASES[name][3]


@functools.lru_cache(maxsize=None)
def case_matrix(name):
    """S float64 [P, P] of a case (treat it as read-only)"""
    gen, args, _, _ = CASES[name]
    S = np.ascontiguousarray(gen(*args), dtype=np.float64)
    assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0)
    if gen is planted_ties:
        h = linkage_average(1.0 - S)[1]
        _, counts = np.unique(h, return_counts=True)
        tied = int(counts[counts > 1].sum())
        assert 4 * tied >= len(h), f"{name}: only {tied} of {len(h)} merge heights are tied"
    S.setflags(write=False)
    return S


def case_pages(name):
    gen, args, _, _ = CASES[name]
    return int(args[0])


def matrix_hash(S):
    return hashlib.sha256(np.ascontiguousarray(S, dtype=np.float64).tobytes()).hexdigest()


def check_hash(golden, name, S):
    """The golden's labels belong to these bytes only; a mismatch fails (it is never a reason to skip)."""
    want = str(golden[f"{name}_sha256"])
    got = matrix_hash(S)
    assert got == want, (f"{name}: the generator no longer builds the matrix the golden was computed from (sha256 {got} != {want}): "
                         "numpy's random stream or the generator changed; regenerate with tests/golden/make_cluster_scale_golden.py")
