"""The fast float64 clustering reference (tests/cluster_reference.py) without a GPU: it is only worth comparing a kernel
with once it is known to be scipy / scikit-learn itself, and its inputs only once they are known to separate the bugs
they were planted for.

Reference of the reference, each compared in bits (children, heights, labels, silhouettes; no tolerance anywhere):
  * oracle/cluster.py (the literal restatement) on the committed linkage_cases.npz / cluster_cases.npz, which themselves
    hold outputs of the real libraries;
  * tests/golden/cluster_scale_cases.npz (scipy `linkage` + scikit-learn `_hc_cut` / `silhouette_score`, written by
    tests/golden/make_cluster_scale_golden.py) on every precomputed-mode case up to 4096 pages and every fallback-mode
    case up to 1100 pages (the float64 row-distance pass in numpy takes seconds beyond that; the GPU test uses the
    golden there);
  * scipy and scikit-learn themselves where they are installed, on every case up to 1100 pages.
Exactness: all of it is float64 with the libraries' own operation order (first minimum of a scan, previous chain element
kept unless strictly beaten, stable sort by height, column-order sums of squares, bincount sums, numpy's pairwise mean).

Mutants, as changes of the reference (cluster_reference.MUTANTS): each must change the labels of a listed n_clusters on
a tie case (planted ties, identity matrices), or, for the scan that stops at index 1024, on the 1030- and 1100-page
cases -- otherwise those cases would not notice a kernel that broke the rule.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402

from oracle import cluster as oc  # noqa: E402

SHORT = {"reference_fallback": "fb", "precomputed": "pre"}
CPU_FALLBACK_MAX = 1100


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_scale_cases.npz"))


@functools.lru_cache(maxsize=None)
def _result(name, mode):
    """cluster_reference.cluster of a case for its listed n_clusters, computed once"""
    S = R.case_matrix(name)
    R.check_hash(_golden(), name, S)
    return R.cluster(S, R.listed_ks(name, mode), mode)


def _cpu_cases(max_fallback=CPU_FALLBACK_MAX, max_pages=4096):
    return [(n, m) for n, c in R.CASES.items() for m in c[2]
            if R.case_pages(n) <= max_pages and (m == "precomputed" or R.case_pages(n) <= max_fallback)]


def test_equals_the_oracle_on_the_existing_linkage_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "linkage_cases.npz"))
    tags = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_D")})
    assert tags
    for t in tags:
        D = g[t + "_D"]
        P = D.shape[0]
        for mode, zkey, labkey in (("reference_fallback", "_Z", "_lab"), ("precomputed", "_Zpre", "_labpre")):
            Y = R.pdist_rows(D) if mode == "reference_fallback" else D
            y = oc.pdist_rows_euclidean(D) if mode == "reference_fallback" else oc.squareform_to_condensed(D)
            assert np.array_equal(Y[np.triu_indices(P, 1)], y), (t, mode)
            children, heights = R.linkage_average(Y)
            Z = oc.linkage_average(y, P)
            assert np.array_equal(children, Z[:, :2].astype(np.int64)) and np.array_equal(heights, Z[:, 2]), (t, mode)
            assert np.array_equal(children, g[t + zkey][:, :2].astype(np.int64)) and np.array_equal(heights, g[t + zkey][:, 2]), (t, mode)
            for k in range(2, min(10, P) + 1):
                assert np.array_equal(R.cut(children, k), g[f"{t}{labkey}{k}"]), (t, mode, k)
        res = R.cluster(1.0 - D, None, "reference_fallback")
        for k, sc in res["scores"]:
            assert sc == oc.silhouette_precomputed(D, oc.agglomerative_labels(D, k)), (t, k)


def test_equals_the_oracle_on_the_existing_cluster_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "cluster_cases.npz"))
    checked = 0
    for c in range(int(g["n_cases"])):
        if f"c{c}_none" in g:
            continue  # n_clusters above the page count: the reference returns None before it clusters
        S = g[f"c{c}_S"]
        fixed = int(g[f"c{c}_fixed"])
        names = [f"page_{i:03d}.png" for i in range(S.shape[0])]
        for mode in R.MODES:
            want = oc.cluster_images(S.copy(), names, n_clusters=None if fixed < 0 else fixed, mode=mode)
            res = R.cluster(S, None if fixed < 0 else fixed, mode)
            labels, k = (res["auto_labels"], res["auto_k"]) if fixed < 0 else (res["labels"][fixed], fixed)
            assert k == want["n_clusters"] and labels.tolist() == want["labels"], (c, mode)
            if mode == "reference_fallback":
                assert labels.tolist() == g[f"c{c}_labels"].tolist() and k == int(g[f"c{c}_k"]), c
        checked += 1
    assert checked >= 5


@pytest.mark.parametrize("name,mode", _cpu_cases())
def test_equals_the_scale_golden(name, mode):
    g, m = _golden(), SHORT[mode]
    res = _result(name, mode)
    for k in R.listed_ks(name, mode):
        assert np.array_equal(res["labels"][k], g[f"{name}_{m}_lab{k}"]), (name, mode, k)
        assert len(np.unique(res["labels"][k])) == k
    S = R.case_matrix(name)
    want_k = list(range(2, min(R.max_auto_k(S), S.shape[0] - 1) + 1))
    assert [k for k, _ in res["scores"]] == want_k == [k for k in range(2, 11) if f"{name}_{m}_sil{k}" in g]
    for k, sc in res["scores"]:
        assert sc == float(g[f"{name}_{m}_sil{k}"]), (name, mode, k)
    assert res["auto_k"] == int(g[f"{name}_{m}_k"])
    assert np.array_equal(res["auto_labels"], g[f"{name}_{m}_labauto"])


def test_the_identity_cases_take_the_three_cluster_branch():
    for name in ("eye5", "eye1500"):
        S = R.case_matrix(name)
        assert R.max_auto_k(S) == 3
        res = _result(name, "precomputed")
        assert res["scores"] == [(2, 0.0), (3, 0.0)] and res["auto_k"] == 2
        assert np.all(res["heights"] == res["heights"][0])


def test_singleton_clusters_reach_the_silhouette():
    """precomputed mode: the outliers are at distance 1 from everything and split off one by one (0/0 -> 0 in the
    silhouette); in fallback mode their ROWS are nearly equal, so they merge with each other first and no cut up to 10
    isolates one"""
    res = _result("singletons130", "precomputed")
    sizes = [np.bincount(R.cut(res["children"], k)).min() for k in (6, 10)]
    assert sizes == [1, 1] and len(res["scores"]) == 9


@pytest.mark.parametrize("name,mode", _cpu_cases(max_pages=CPU_FALLBACK_MAX))
def test_equals_scipy_and_scikit_learn(name, mode):
    pytest.importorskip("scipy")
    pytest.importorskip("sklearn")
    import warnings

    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    from sklearn.cluster import AgglomerativeClustering

    S = R.case_matrix(name)
    D = 1.0 - S
    res = _result(name, mode)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy remarks that the rows of D look like a distance matrix: they are, as in the reference
        Z = linkage(squareform(D, checks=False), "average") if mode == "precomputed" else linkage(D, "average", "euclidean")
        children, heights = res["children"], res["heights"]
        assert np.array_equal(children, Z[:, :2].astype(np.int64)), (name, mode)
        assert np.array_equal(heights, Z[:, 2]), (name, mode)
        kw = {"metric": "precomputed"} if mode == "precomputed" else {}
        for k in R.listed_ks(name, mode):
            real = AgglomerativeClustering(n_clusters=k, linkage="average", **kw).fit(D).labels_
            assert np.array_equal(res["labels"][k], real), (name, mode, k)


@functools.lru_cache(maxsize=None)
def _changed_by(mutant, name, mode):
    """the listed n_clusters of a case whose labels a mutant changes"""
    if mode == "reference_fallback":
        pytest.skip("mutants are evaluated on the distance matrix itself")
    S = R.case_matrix(name)
    true = _result(name, mode)["labels"]
    _, children, _ = R.tree(S, mode, **R.MUTANTS[mutant])
    return [k for k in R.listed_ks(name, mode) if not np.array_equal(R.cut(children, k), true[k])]


@pytest.mark.parametrize("mutant,names", [
    ("highest_index_wins", R.TIE_CASES),
    ("previous_not_preferred", ("ties96", "ties1030")),
    ("unstable_height_sort", ("ties96", "eye5", "eye1500")),
    ("scan_stops_at_1024", ("ties1030", "blocked1100", "blocked1025")),
])
def test_mutants_change_labels(mutant, names):
    for name in names:
        changed = _changed_by(mutant, name, "precomputed")
        print(f"{mutant:24s} {name:12s} changes n_clusters {changed}")
        assert changed, (mutant, name)


def test_planted_ties_tie():
    for name in ("ties96", "ties1030"):
        h = _result(name, "precomputed")["heights"]
        _, counts = np.unique(h, return_counts=True)
        assert 4 * counts[counts > 1].sum() >= len(h)
