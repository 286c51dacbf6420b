"""K16, the silhouette over the vector table, without a GPU: the float64 restatement (tests/silhouette_reference.py) against
scikit-learn and the page side's oracle, pick_n_clusters, the header and the refusals that come before any engine."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_reference as K  # noqa: E402
import silhouette_reference as S  # noqa: E402

from multimodal_embeddings_amd import region_compare as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_exports_carry_the_silhouette():
    from multimodal_embeddings_amd import _lib, build

    with open(os.path.join(ROOT, "include", "mme.h")) as fh:
        header = fh.read()
    for name in ("mme_silhouette", "mme_silhouette_rows"):
        assert re.search(r"\bint %s\(mme_ctx\*" % name, header), name
        assert name in _lib.EXPORTS
    assert "#define MME_ABI_VERSION 2" in header
    body = re.search(r"typedef struct mme_silhouette_out \{(.*?)\} mme_silhouette_out;", header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in _lib._SilhouetteOut._fields_] == ["sample", "cluster", "score", "info", "sums", "counts"]
    assert "silhouette.hip" in build.SOURCES


def _case(n, d, seed):
    """seeded bf16 unit rows around 6 centres, labels 0..7 with some rows moved to a neighbour, cluster 6 empty and cluster 7
    one row"""
    k = 8
    xb, lab = S.planted(n, d, 6, seed, noise=1.0)
    rng = np.random.default_rng(seed + 1)
    moved = rng.choice(n, size=n // 10, replace=False)
    lab = lab.copy()
    lab[moved] = (lab[moved] + 1) % 6
    lab[n // 3] = 7
    return xb, lab, k


@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("n", [300, 1024])
def test_the_two_forms_scikit_learn_and_the_page_oracle_agree(n, d):
    from sklearn.metrics import silhouette_samples, silhouette_score

    from oracle.cluster import silhouette_precomputed

    xb, lab, k = _case(n, d, seed=n + d)
    ref = S.by_sums(xb, lab, k)
    assert ref["counts"][6] == 0 and ref["counts"][7] == 1 and ref["info"].tolist() == [n, 7]
    assert ref["sample"][n // 3] == 0.0 and np.isnan(ref["cluster"][6]) and ref["cluster"][7] == 0.0
    pairs = S.all_pairs(xb, lab, k)
    x64 = K.bf16_to_f64(xb)
    D = 1.0 - x64 @ x64.T
    np.fill_diagonal(D, 0.0)
    _, dense = np.unique(lab, return_inverse=True)  # scikit-learn and the oracle want labels without a hole
    sk = silhouette_samples(D, dense, metric="precomputed")
    worst = {"sums - pairs": float(np.abs(ref["sample"] - pairs).max()), "pairs - sklearn": float(np.abs(pairs - sk).max()),
             "sums - sklearn": float(np.abs(ref["sample"] - sk).max())}
    means = {"sums": ref["score"], "pairs": float(pairs.mean()), "sklearn": float(sk.mean()), "oracle": silhouette_precomputed(D, dense.astype(np.int64))}
    print(n, d, worst, means)
    assert max(worst.values()) <= 1e-12, worst
    assert max(means.values()) - min(means.values()) <= 1e-12, means
    # recorded only: scikit-learn's own cosine metric renormalises the rows, which bf16 rows are not exactly
    print("to metric='cosine':", abs(silhouette_score(x64, dense, metric="cosine") - ref["score"]))


def test_rows_of_no_cluster_and_degenerate_partitions():
    xb, lab, k = _case(300, 64, seed=5)
    ref = S.by_sums(xb, lab, k)
    out = lab.copy()
    out[[0, 17]] = [-1, k]
    got = S.by_sums(xb, out, k)
    assert np.isnan(got["sample"][[0, 17]]).all() and got["info"].tolist() == [298, 7]
    keep = np.ones(300, dtype=bool)
    keep[[0, 17]] = False
    again = S.by_sums(xb[keep], lab[keep], k)  # leaving the rows out is the same thing
    assert np.array_equal(got["sample"][keep], again["sample"]) and got["score"] == again["score"]
    assert not np.array_equal(got["sample"][keep], ref["sample"][keep])
    one = S.by_sums(xb, np.zeros(300, dtype=np.int32), 2)  # one cluster with members: no score, samples 0
    assert np.isnan(one["score"]) and one["info"].tolist() == [300, 1] and not one["sample"].any() and np.isnan(one["cluster"][1])
    none = S.by_sums(xb, np.full(300, -1, dtype=np.int32), 2)
    assert np.isnan(none["score"]) and none["info"].tolist() == [0, 0] and np.isnan(none["sample"]).all()


def test_pick_n_clusters_is_the_page_sides_rule():
    nan = float("nan")
    assert rc.pick_n_clusters({2: 0.1, 3: 0.5, 4: 0.3}) == 3
    assert rc.pick_n_clusters({4: 0.3, 2: 0.1, 3: 0.5}) == 3  # k ascending, whatever the dict's order
    assert rc.pick_n_clusters({2: 0.5, 3: 0.5, 4: 0.5}) == 2  # strict >: the first among equals
    assert rc.pick_n_clusters({2: 0.2, 3: 0.5, 4: 0.5}) == 3
    assert rc.pick_n_clusters({2: nan, 3: 0.1, 4: None, 5: 0.05}) == 3  # no score: skipped
    assert rc.pick_n_clusters({3: nan, 4: None}) == 3  # nothing to compare: the first k
    assert rc.pick_n_clusters({2: -1.0, 3: -1.0}) == 2  # -1 is where the best starts, and it is not above itself
    assert rc.pick_n_clusters({2: -1.0, 3: -0.5}) == 3
    assert rc.pick_n_clusters({5: 0.9}) == 5
    with pytest.raises(ValueError):
        rc.pick_n_clusters({})
    for scores in ({2: 0.1, 3: 0.5, 4: 0.3}, {2: nan, 3: 0.1, 4: None}, {3: nan}):
        assert rc.pick_n_clusters(scores) == S.pick(scores)
    # the rule of oracle/cluster.py, cluster_images: `best_score, best_k = -1, 2` and `if score > best_score`
    src = inspect.getsource(__import__("oracle.cluster", fromlist=["cluster_images"]).cluster_images)
    assert "best_score, best_k = -1, 2" in src and "if score > best_score" in src


class _Rows:
    """a collection of n regions; nothing here may reach the GPU"""

    def __init__(self, n):
        self.n = n

    def get(self, include=None, where=None):
        return {"ids": [f"r{i}" for i in range(self.n)], "metadatas": [{"is_region": True}] * self.n, "embeddings": [[1.0] + [0.0] * 63] * self.n}


def test_python_side_refusals_come_before_any_engine():
    col = _Rows(5)
    for kw, msg in [(dict(k_range=range(6, 9)), r"no k in 2\.\.5"), (dict(k_range=[0, 1]), r"no k in 2\.\.5"), (dict(k_range=[]), "no k in"),
                    (dict(n_init=0), "n_init = 0"), (dict(max_iter=1001), r"0\.\.1000")]:
        with pytest.raises(ValueError, match=msg):
            rc.cluster_regions(col, None, **kw)
        with pytest.raises(ValueError, match=msg):
            rc.kmeans_regions(col, n_clusters=None, **kw)
    assert rc._clip_k_range(range(2, 11), 5) == [2, 3, 4, 5] and rc._clip_k_range([7, 3, 3, 1], 7) == [3, 7]
    none = rc.cluster_regions(_Rows(0), None)
    assert none["n_regions"] == 0 and none["clusters"] == [] and "k_scores" not in none
    for labels, msg in [([0, 0, 0, 0, 0], "1 cluster"), ([-1, -1, 3, 3, -1], "1 cluster"), ([-1] * 5, "0 cluster"), ([0, 1, 0], "3 labels for 5 regions"),
                        ([0.0, 1.0, 0.0, 1.0, 1.0], "integers")]:
        with pytest.raises(ValueError, match=msg):
            rc.silhouette_regions(col, labels)
    sig = inspect.signature(rc.kmeans_regions).parameters
    assert list(sig["k_range"].default) == list(range(2, 11)) and sig["silhouette"].default is False and sig["silhouette_samples"].default is False
    sig = inspect.signature(rc.cluster_regions).parameters
    assert list(sig["k_range"].default) == list(range(2, 11)) and sig["silhouette"].default is False


def test_the_committed_fixture_keeps_its_margins():
    """what "choosing k" in tests/test_gpu_silhouette.py asserts on the GPU's bits holds on the rows normalised here"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_silhouette_case as M

    g = np.load(os.path.join(S.GOLDEN, "silhouette_choose.npz"))
    c = S.CHOOSE
    assert g["x"].shape == (c["n"], c["d"]) and g["x"].dtype == np.float32
    assert np.array_equal(g["x"], M.rows_of(int(g["data_seed"])))
    runs, picked = S.choose_k(M.unit_bits(g["x"]), c["k_range"], int(g["seed"]), c["max_iter"])
    assert sorted(runs) == list(c["k_range"]) and picked == int(g["picked"]) == c["centres"]
    assert min(v["run"]["gap"] for v in runs.values()) > 4 * K.delta(c["d"]) and all(v["run"]["converged"] for v in runs.values())
    scores = sorted((v["sil"]["score"] for v in runs.values()), reverse=True)
    assert scores[0] - scores[1] > 1e-6
