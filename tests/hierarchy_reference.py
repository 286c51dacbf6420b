"""float64 reference of the cluster hierarchy (K19), and the inputs its tests share.

Over s64 = the float64 dot product of the bf16 rows (tests/duplicates_reference.py): the core similarities by sorting, the
mutual-reachability weights M, Kruskal's maximal spanning forest under the strict order "m descending, lo ascending, hi
ascending", and the cut at a threshold through scipy's connected components.  `boruvka` restates the rounds the kernels run
(row key, component choice, the mutual-choice rule) in numpy: the executable statement of the tie rule, with the three ways
of getting it wrong as `mutant`.

The inputs are the six cases of tests/density_reference.py with their thresholds, at min_samples 3 and 8, without groups and
with the 7-page ids.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as R  # noqa: E402
import duplicates_reference as DR  # noqa: E402

MIN_SAMPLES = (3, 8)
ABOVE, BELOW = 1.5, -2.0  # the core similarity at min_samples = 1, and of a row with too few admissible partners
COMBOS = [(n, d, seed, ms, grouped) for (n, d, seed) in R.CASES for ms in MIN_SAMPLES for grouped in (False, True)]


def core_similarity(S, adm, min_samples):
    """float64 [n]: the (min_samples - 1)-th largest admissible similarity of every row"""
    n = len(S)
    if min_samples == 1:
        return np.full(n, ABOVE)
    k = min_samples - 1
    Sa = -np.sort(-np.where(adm, S, -np.inf), axis=1)
    col = Sa[:, k - 1] if k <= n else np.full(n, -np.inf)
    return np.where(np.isfinite(col), col, BELOW)


def mutual(S, adm, core):
    """float64 [n, n]: min(core_i, core_j, s_ij) on the admissible pairs, -inf elsewhere"""
    return np.where(adm, np.minimum(np.minimum(core[:, None], core[None, :]), S), -np.inf)


def kruskal(M, adm):
    """(edges int64 [E, 2] as (lo, hi), weights float64 [E]) of the maximal spanning forest under the strict order, in that order"""
    lo, hi = np.nonzero(np.triu(adm, 1))
    w = M[lo, hi]
    order = np.lexsort((hi, lo, -w))
    top = list(range(len(M)))

    def find(x):
        while top[x] != x:
            top[x] = top[top[x]]
            x = top[x]
        return x

    edges, weights = [], []
    for a, b, m in zip(lo[order].tolist(), hi[order].tolist(), w[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            top[max(ra, rb)] = min(ra, rb)
            edges.append((a, b))
            weights.append(m)
    return np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(weights, dtype=np.float64)


def components(adm_or_edges, n=None):
    """labels (the smallest member) of the components of a bool adjacency matrix, or of an edge list over n rows"""
    from scipy.sparse import coo_matrix, csr_matrix
    from scipy.sparse.csgraph import connected_components

    if n is None:
        n = len(adm_or_edges)
        g = csr_matrix(adm_or_edges)
    else:
        e = np.asarray(adm_or_edges).reshape(-1, 2)
        g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
    _, comp = connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp]


def cut(edges, weights, core, threshold):
    """(labels, kind): the components of the edges with weight >= threshold among the rows with core >= threshold (the id is
    the smallest member), -1 / 0 for every other row"""
    n = len(core)
    keep = np.asarray(weights) >= threshold
    lab = components(np.asarray(edges).reshape(-1, 2)[keep], n)
    is_core = np.asarray(core) >= threshold
    return np.where(is_core, lab, -1), np.where(is_core, 2, 0)


def boruvka(M, adm, mutant=None):
    """The rounds of the kernels in numpy.  -> (set of (lo, hi), rounds that emitted, cycles met).
    mutant: "other_root" -- a component chooses by (m, the other component's id) instead of the real endpoints;
            "j_descending" -- among a row's equal weights the highest j; "no_mutual_rule" -- both ends emit a shared edge."""
    n = len(M)
    comp = np.arange(n)
    top = list(range(n))

    def find(x):
        while top[x] != x:
            top[x] = top[top[x]]
            x = top[x]
        return x

    edges, rounds, cycles = [], 0, 0
    while True:
        ok = adm & (comp[:, None] != comp[None, :])
        has = ok.any(1)
        if not has.any():
            break
        Mm = np.where(ok, M, -np.inf)
        best = Mm.max(1)
        attain = ok & (Mm == best[:, None])
        j = n - 1 - np.argmax(attain[:, ::-1], axis=1) if mutant == "j_descending" else np.argmax(attain, axis=1)  # the row key
        chosen = {}
        for c in np.unique(comp[has]).tolist():
            rows = np.flatnonzero(has & (comp == c))
            rows = rows[best[rows] == best[rows].max()]
            if mutant == "other_root":
                i = int(rows[np.argmin(comp[j[rows]])])
                chosen[c] = (min(i, int(j[i])), max(i, int(j[i])))
            else:
                chosen[c] = min((min(int(i), int(j[i])), max(int(i), int(j[i]))) for i in rows)
        emitted = 0
        for c, (lo, hi) in chosen.items():
            other = int(comp[hi]) if comp[lo] == c else int(comp[lo])
            if mutant != "no_mutual_rule" and other < c and chosen.get(other) == (lo, hi):
                continue
            edges.append((lo, hi))
            emitted += 1
            a, b = find(lo), find(hi)
            if a == b:
                cycles += 1
            else:
                top[max(a, b)] = min(a, b)
        comp = np.array([find(x) for x in range(n)])
        rounds += 1
        if emitted == 0 or rounds > 64:
            break
    return edges, rounds, cycles


def one_hot(n, classes, d=64):
    """x_i = e_(i mod classes): (float32 rows, bf16 tensor), exact in bf16"""
    x = np.zeros((n, d))
    x[np.arange(n), np.arange(n) % classes] = 1.0
    return DR.to_bf16(x)


@functools.lru_cache(maxsize=None)
def case(n, d, seed, min_samples, grouped=False):
    """One combination, computed once and shared (read-only): density_reference.table's fields plus min_samples, group (or
    None), adm, core, M and Kruskal's tree (edges, weights)."""
    t = R.table(n, d, seed)
    group = R.group_ids(n, seed) if grouped else None
    adm = DR.admissible(n, group)
    core = core_similarity(t["S"], adm, min_samples)
    M = mutual(t["S"], adm, core)
    edges, weights = kruskal(M, adm)
    return {**t, "min_samples": min_samples, "group": group, "adm": adm, "core": core, "M": M, "edges": edges, "weights": weights}


def same_partition(a, b):
    """two label vectors (-1 = noise) describe the same noise set and the same partition of the other rows"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    keep = a >= 0
    pairs = set(zip(a[keep].tolist(), b[keep].tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))
