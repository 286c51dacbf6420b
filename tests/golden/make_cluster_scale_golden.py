"""Writes tests/golden/cluster_scale_cases.npz: what scipy and scikit-learn return for the large and tie-heavy page
matrices of tests/cluster_reference.py (numpy, scipy and scikit-learn only; run from anywhere).

The matrices are not stored: each case is rebuilt from its seed, and the file holds sha256(S.tobytes()) so that a test
notices a changed random stream.  Per case and mode ("fb" = reference_fallback, euclidean distances between the rows of
D = 1 - S; "pre" = D itself as the distance matrix):
  {case}_{mode}_lab{k}   int16 labels for each listed n_clusters
  {case}_{mode}_sil{k}   silhouette_score(D, labels, metric='precomputed') for k = 2..max k, where defined
  {case}_{mode}_k, {case}_{mode}_labauto   the k of the strict-> argmax (wrc:482-490) and its labels
The tree is computed once per case and mode with scipy's `linkage` and cut with scikit-learn's `_hc_cut`; on every case
of at most 1100 pages that is asserted to equal AgglomerativeClustering(...).fit(D).labels_ for every listed k.  The best
and the second-best silhouette must differ by more than 1e-9 (a rounding-level difference cannot move the chosen k); the
identity matrices are the exception that needs none: every silhouette term there is an exact 0.
"""
import os
import sys
import time

import numpy as np
import scipy
import sklearn
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import squareform
from sklearn.cluster import AgglomerativeClustering
from sklearn.cluster._agglomerative import _hc_cut
from sklearn.metrics import silhouette_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cluster_reference as R  # noqa: E402  (the seeded generators only)

SHORT = {"reference_fallback": "fb", "precomputed": "pre"}


def main():
    out = {"versions": np.array(f"numpy {np.__version__} scipy {scipy.__version__} scikit-learn {sklearn.__version__}")}
    for name, (_, _, modes, _) in R.CASES.items():
        S = R.case_matrix(name)
        P = S.shape[0]
        out[f"{name}_sha256"] = np.array(R.matrix_hash(S))
        D = 1.0 - S
        max_k = R.max_auto_k(S)
        for mode in modes:
            t0 = time.time()
            m = SHORT[mode]
            if mode == "precomputed":
                Z = linkage(squareform(D, checks=False), "average")
            else:
                Z = linkage(D, "average", "euclidean")
            children = Z[:, :2].astype(np.intp)
            for k in R.listed_ks(name, mode):
                lab = _hc_cut(k, children, P)
                if P <= 1100:
                    kw = {"metric": "precomputed"} if mode == "precomputed" else {}
                    real = AgglomerativeClustering(n_clusters=k, linkage="average", **kw).fit(D).labels_
                    assert np.array_equal(lab, real), (name, mode, k)
                assert lab.max() < 2 ** 15
                out[f"{name}_{m}_lab{k}"] = lab.astype(np.int16)
            best_score, best_k, scores = -1, 2, []
            for k in range(2, max_k + 1):
                lab = _hc_cut(k, children, P)
                if not 1 < len(np.unique(lab)) < P:
                    continue
                score = float(silhouette_score(D, lab, metric="precomputed"))
                out[f"{name}_{m}_sil{k}"] = np.array(score)
                scores.append(score)
                if score > best_score:
                    best_score, best_k = score, k
            top = sorted(scores, reverse=True)
            gap = top[0] - top[1] if len(top) > 1 else np.inf
            assert gap > 1e-9 or all(s == 0.0 for s in scores), (name, mode, scores)
            out[f"{name}_{m}_k"] = np.array(best_k)
            out[f"{name}_{m}_labauto"] = _hc_cut(best_k, children, P).astype(np.int16)
            print(f"{name:14s} {mode:18s} P={P:5d} k={best_k:2d} gap={gap:.3e} {time.time() - t0:6.1f} s", flush=True)
    path = os.path.join(HERE, "cluster_scale_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
