"""float64 / scipy reference of the density clusters (K18, DBSCAN), and the inputs its tests share.

The neighbour relation is K14's (tests/duplicates_reference.py): against s64 = the float64 dot product of the bf16 rows, with
delta = 2 * d * 2^-24, a pair with s64 >= tau + delta is a neighbour pair, one with s64 < tau - delta is none, in between either
answer is right.  So every input here comes with a threshold whose dead zone holds no admissible pair, and then counts, core
rows, clusters and the noise set have exactly one right answer.  A border row's cluster has one right answer unless a core
neighbour of ANOTHER cluster lies within 2 delta of its best one (`ambiguous`); its partner unless its two best core
neighbours lie within 2 delta (`idx_ties`).
"""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duplicates_reference as DR  # noqa: E402

# (n, d, seed) of the main cases: gaps of >= 4 delta, no dead-zone pair, no ambiguous border row (test_density_cpu.py asserts it)
CASES = [(203, 64, 1), (203, 64, 2), (331, 128, 1), (515, 256, 1), (515, 768, 1), (643, 1024, 1)]
PAGES = 7  # group ids of the grouped variants: default_rng(1000 + seed).integers(0, PAGES, n)


def blobs(n, d, seed, per=16):
    """ceil(n / per) blobs of `per` rows around unit centres, at radii drawn per row, so that a blob has a dense middle (core
    rows), a sparse rim (border rows) and stragglers (noise); the last two rows of every fourth blob are bridges, half way
    to the next centre, which chain two blobs under single linkage but are not core.  Rows permuted, rounded to bf16.
    (Random walks are useless here: their graph has degree <= 2.)"""
    rng = np.random.default_rng(seed)
    k = math.ceil(n / per)
    C = rng.standard_normal((k, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    x = np.empty((n, d))
    for i in range(n):
        c, r = divmod(i, per)
        if c % 4 == 0 and r >= per - 2 and c + 1 < k:
            g = rng.standard_normal(d)
            x[i] = C[c] + C[c + 1] + 0.2 * g / np.sqrt(d)
        else:
            s = 0.25 + 0.8 * rng.random()
            g = rng.standard_normal(d)
            x[i] = C[c] + s * g / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x[rng.permutation(n)]
    return DR.to_bf16(x)


def reference(x32, tau, min_samples, group=None, S=None):
    """Everything K18 returns, from float64: dict of labels, kind, count, border_idx, border_sim, summary, plus S, adm,
    `ambiguous` and `idx_ties` (bool [n], see the head of this file) and `two_clusters` (border rows with core neighbours in
    more than one cluster)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    x32 = np.asarray(x32)
    n, d = x32.shape
    S = DR.similarity(x32) if S is None else S
    adm = DR.admissible(n, group)
    E = adm & (S >= tau)
    count = E.sum(1).astype(np.int32)
    core = count + 1 >= min_samples
    Ec = E & core[:, None] & core[None, :]
    ncomp, comp = connected_components(csr_matrix(Ec), directed=False)
    smallest = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(smallest, comp[core], np.flatnonzero(core))
    labels = np.where(core, smallest[comp], -1).astype(np.int64)
    Sc = np.where(E & core[None, :], S, -np.inf)  # a row's core neighbours
    border = ~core & (Sc > -np.inf).any(1)
    best = np.argmax(Sc, axis=1)  # argmax: the lowest index among equal values
    border_idx = np.where(border, best, -1).astype(np.int32)
    border_sim = np.where(border, Sc[np.arange(n), best], 0.0)
    labels[border] = labels[best[border]]
    kind = np.where(core, 2, np.where(border, 1, 0)).astype(np.int32)
    dl2 = 2 * DR.delta(d)
    ambiguous = np.zeros(n, dtype=bool)
    idx_ties = np.zeros(n, dtype=bool)
    two_clusters = np.zeros(n, dtype=bool)
    for r in np.flatnonzero(border):
        near = np.flatnonzero(Sc[r] > -np.inf)
        two_clusters[r] = len(set(labels[near].tolist())) > 1
        close = near[Sc[r, near] >= border_sim[r] - dl2]
        idx_ties[r] = len(close) > 1
        ambiguous[r] = (labels[close] != labels[r]).any()
    sizes = np.bincount(labels[labels >= 0], minlength=n) if n else np.zeros(0, dtype=np.int64)
    pairs = int(np.triu(E, 1).sum())
    summary = np.array([pairs, int((sizes > 0).sum()), int(core.sum()), int(border.sum()), int((kind == 0).sum()),
                        int(sizes.max()) if n else 0], dtype=np.int64)
    return {"labels": labels.astype(np.int32), "kind": kind, "count": count, "border_idx": border_idx, "border_sim": border_sim,
            "summary": summary, "S": S, "adm": adm, "ambiguous": ambiguous, "idx_ties": idx_ties, "two_clusters": two_clusters}


@functools.lru_cache(maxsize=None)
def table(n, d, seed):
    """rows, their float64 similarities and the threshold of one main case, computed once and shared (read-only)"""
    x32, xb = blobs(n, d, seed)
    S = DR.similarity(x32)
    tau, gap = DR.widest_gap(S)
    return {"n": n, "d": d, "seed": seed, "x32": x32, "xb": xb, "S": S, "tau": tau, "gap": gap}


def group_ids(n, seed, pages=PAGES):
    return np.random.default_rng(1000 + seed).integers(0, pages, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(n, d, seed, min_samples, grouped=False):
    """One main case with its reference (treat it as read-only): table()'s fields plus min_samples, group (or None), ref, and
    `dead`, the admissible pairs inside the dead zone."""
    t = table(n, d, seed)
    group = group_ids(n, seed) if grouped else None
    ref = reference(t["x32"], t["tau"], min_samples, group, S=t["S"])
    return {**t, "min_samples": min_samples, "group": group, "ref": ref,
            "dead": DR.dead_zone_pairs(ref["S"], ref["adm"], t["tau"], DR.delta(d))}


def check_fixture(c):
    """the conditions under which the reference is the only right answer (a fixture error, never a skip)"""
    ref, dl = c["ref"], DR.delta(c["d"])
    assert c["dead"] == 0, f"fixture: {c['dead']} admissible pairs inside the dead zone of tau = {c['tau']}"
    assert c["gap"] >= 4 * dl, f"fixture: gap = {c['gap'] / dl:.1f} delta"
    assert not ref["ambiguous"].any(), f"fixture: border rows {np.flatnonzero(ref['ambiguous'])} have two clusters within 2 delta"
    n_border, ties = int((ref["kind"] == 1).sum()), int(ref["idx_ties"].sum())
    assert ties <= 4 and ties <= 0.05 * n_border, f"fixture: {ties} of {n_border} border rows have two best core neighbours within 2 delta"
