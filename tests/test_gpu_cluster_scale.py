"""K11 (`linkage_and_cut`, csrc/cluster.hip) past the 1024 lanes of its one workgroup, up to the 4096-page limit, and on
matrices whose labels the tie rules alone decide -- against scipy and scikit-learn.

The linkage is one workgroup of 1024 lanes whose scans all run `for (i = tid; i < P; i += 1024)`: from 1025 pages on a
lane takes a second trip through the first-live search, the nearest-neighbour scan, the Lance-Williams update, the leaf
labelling, the silhouette rows and the rank sort; 2049 and 4096 pages make two and four full trips.

Reference: tests/golden/cluster_scale_cases.npz -- scipy `linkage(..., 'average')` cut with scikit-learn's `_hc_cut`
(asserted equal to AgglomerativeClustering up to 1100 pages when the file was written) and scikit-learn's
`silhouette_score`, per case and mode; the matrices are rebuilt from their seeds (tests/cluster_reference.py) and their
sha256 is asserted first.  For precomputed mode up to 2049 pages the float64 restatement of tests/cluster_reference.py
runs in the test as well, so that a failure says which side moved.  Labels, the chosen k and the list of evaluated k
compare exactly; silhouettes within 1e-13 absolute, the project's bound from test_large_seeded_matrices_vs_oracle (all
arithmetic is f64 in the libraries' operation order, so the expected difference is 0).

Cases (cluster_reference.CASES), both modes each: blocked random matrices of 1025, 1100, 2049 and 4096 pages; planted ties
(entries in {0, 1/4, 1/2, 3/4}, one page in ten an exact copy of another; at least a quarter of the merge heights tied)
of 96 and 1030 pages; the identity matrix of 5 and 1500 pages (every distance equal, the `nonzero_pairs < 10` branch,
every silhouette 0, k stays 2); 130 pages with five outliers (one-member clusters in the silhouette).  Fixed n_clusters
2, 3, 10 (2, 3 at five pages; 5, 7 more on the tie cases), {1, 11, 64, P-1, P} at 130 and 1025 pages, {11, 1000, 4095, 4096} at 4096 pages: the heap of
`_hc_cut` grows to P entries.  Mutants (asserted in tests/test_cluster_reference_cpu.py to change labels on these cases):
lowest-index tie rule reversed, previous chain element not preferred on a tie, unstable height sort, scan stopping at
index 1024.

Measured on the MI355X: one fallback-mode call at 4096 pages (the strided `pdist_rows` pass included) takes 0.86 s, one
at 2049 pages 0.21 s, so the fallback case stays at the limit of 4096 pages, with fewer fixed n_clusters than the other
cases (cluster_reference.FALLBACK_KS); a precomputed-mode call at 4096 pages takes 0.08 s with n_clusters fixed and 0.33 s
with the silhouette search.  Whole module 9.5 s; slowest case 3.8 s (4096 pages, fallback: two device calls, the rest is
building, hashing and copying the 128 MiB matrix), every other case below 1 s.  Largest |silhouette - golden| observed,
per case and mode (printed by the test): 0 on every one of the 18 -- the device's silhouettes are the libraries' bits.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHORT = {"reference_fallback": "fb", "precomputed": "pre"}
SIL_TOL = 1e-13
CPU_REFERENCE_MAX = 2049


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cluster_scale_cases.npz"))


_device = {}


def _matrix(golden, name):
    """(S on the host, S on the device) of a case, its hash checked against the golden's"""
    S = R.case_matrix(name)
    if name not in _device:
        R.check_hash(golden, name, S)
        _device[name] = torch.from_numpy(np.array(S)).cuda()
    return S, _device[name]


def _check_case(engine, golden, name, mode):
    S, Sd = _matrix(golden, name)
    m = SHORT[mode]
    P = S.shape[0]
    for k in R.listed_ks(name, mode):
        lab, kk, _ = engine.cluster_pages(Sd, k, mode)
        assert kk == k, (name, mode, k, kk)
        assert np.array_equal(np.asarray(lab), golden[f"{name}_{m}_lab{k}"]), (name, mode, k)
    lab, kk, scores = engine.cluster_pages(Sd, None, mode)
    assert kk == int(golden[f"{name}_{m}_k"]), (name, mode, kk)
    assert np.array_equal(np.asarray(lab), golden[f"{name}_{m}_labauto"]), (name, mode)
    max_k = R.max_auto_k(S)
    assert [k for k, _ in scores] == list(range(2, max_k + 1)), (name, mode, scores)
    diffs = [abs(sc - float(golden[f"{name}_{m}_sil{k}"])) for k, sc in scores]
    print(f"{name:14s} {mode:18s} P={P:5d} k={kk:2d} max |silhouette - golden| = {max(diffs):.3e}")
    assert max(diffs) <= SIL_TOL, (name, mode, diffs)
    return scores


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_labels_k_and_silhouettes_equal_scipy_and_scikit_learn(engine, golden, name, mode):
    assert mode in R.CASES[name][2]
    _check_case(engine, golden, name, mode)
    if mode == "precomputed" and R.case_pages(name) <= CPU_REFERENCE_MAX:
        m = SHORT[mode]
        ref = R.cluster(R.case_matrix(name), R.listed_ks(name, mode), mode)
        for k in R.listed_ks(name, mode):
            assert np.array_equal(ref["labels"][k], golden[f"{name}_{m}_lab{k}"]), ("reference != golden", name, k)
        assert ref["auto_k"] == int(golden[f"{name}_{m}_k"]) and np.array_equal(ref["auto_labels"], golden[f"{name}_{m}_labauto"])
        assert all(sc == float(golden[f"{name}_{m}_sil{k}"]) for k, sc in ref["scores"]), ("reference != golden", name)


def test_identity_keeps_two_clusters(engine, golden):
    for name in ("eye5", "eye1500"):
        for mode in R.MODES:
            _, Sd = _matrix(golden, name)
            _, k, scores = engine.cluster_pages(Sd, None, mode)
            assert k == 2 and scores == [(2, 0.0), (3, 0.0)], (name, mode, scores)


def test_limits_are_refused_and_the_engine_goes_on(engine, golden):
    from multimodal_embeddings_amd._lib import MmeError

    too_many = torch.eye(4097, dtype=torch.float64, device="cuda")
    with pytest.raises(MmeError, match="P=4097"):
        engine.cluster_pages(too_many, None, "precomputed")
    with pytest.raises(MmeError, match="P=4097"):
        engine.cluster_pages(too_many, 3, "reference_fallback")
    del too_many
    _check_case(engine, golden, "eye5", "precomputed")
    for name in ("eye5", "ties96"):
        _, Sd = _matrix(golden, name)
        P = R.case_pages(name)
        with pytest.raises(MmeError, match=f"n_clusters={P + 1}"):
            engine.cluster_pages(Sd, P + 1, "precomputed")
        lab, k, _ = engine.cluster_pages(Sd, P, "precomputed")  # the largest n_clusters that is accepted: one page each
        assert k == P and sorted(lab) == list(range(P))
    _check_case(engine, golden, "ties96", "reference_fallback")


def test_a_small_call_reuses_the_workspace_of_a_large_one(engine, golden):
    _, Sd = _matrix(golden, "blocked4096")
    lab, k, _ = engine.cluster_pages(Sd, 11, "precomputed")
    assert k == 11 and np.array_equal(np.asarray(lab), golden["blocked4096_pre_lab11"])
    for mode in R.MODES:
        _check_case(engine, golden, "ties96", mode)
