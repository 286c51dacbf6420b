"""K17 without a device: the float64 restatement checks itself, the order of the definition is shown to matter, and the host
half of the fit (region_compare.projection_from_moments), the store round trip and project_collection are tested on planted data.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import projection_reference as PJ  # noqa: E402

from multimodal_embeddings_amd import region_compare as RC  # noqa: E402
from multimodal_embeddings_amd import store  # noqa: E402
from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection  # noqa: E402


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_reference_equals_fsum_where_every_sum_is_exact():
    """Values k / 64 with |k| <= 128 are bf16 values; their products are multiples of 2^-12 below 4, and 300 of them add up
    without any rounding in float64.  So the sequential sums of the restatement and math.fsum's correctly rounded sums must agree
    bit for bit -- whatever the block size."""
    rng = np.random.default_rng(5)
    x = rng.integers(-128, 129, (300, 6)) / 64.0
    assert np.array_equal(PJ.bf16_exact(x), x)
    s, g = PJ.moments(x, block=128)
    for a in range(6):
        assert s[a] == math.fsum(x[:, a])
        for c in range(6):
            assert g[a, c] == math.fsum(x[i, a] * x[i, c] for i in range(300))
    assert np.array_equal(PJ.bits(g), PJ.bits(g.T))


def test_bf16_helpers_round_to_nearest_even():
    import torch

    v = np.random.default_rng(6).standard_normal(4096).astype(np.float32) * 3
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(PJ.to_bf16_bits(v), want)
    assert np.array_equal(PJ.bf16_bits_to_f64(want), torch.from_numpy(v).to(torch.bfloat16).double().numpy())


def test_order_sensitivity_of_the_mixed_magnitudes_fixture():
    """The GPU test compares bits with PJ.moments on this fixture.  Here: walking the rows backwards, or one block in place of
    blocks of B, changes bits of the reference gram -- so that comparison tells a wrong order from the right one."""
    x = PJ.mixed_magnitudes()
    assert x.shape == (3 * PJ.BLOCK + 5, 64)
    mag = np.abs(x)
    assert mag.min() >= 2.0 ** -10 and mag.max() <= 2.0 ** 10 and mag.min() < 2.0 ** -9 and mag.max() > 2.0 ** 9
    s, g = PJ.moments(x)
    s_rev, g_rev = PJ.moments(x, reverse=True)
    s_one, g_one = PJ.moments(x, block=x.shape[0])
    assert np.array_equal(PJ.bits(g), PJ.bits(g.T))
    assert (PJ.bits(g) != PJ.bits(g_rev)).any(), "reversing the rows changed no bit"
    assert (PJ.bits(g) != PJ.bits(g_one)).any(), "one block in place of blocks of B changed no bit"
    # the column sums cannot tell: 8-bit values over 20 binades, 3077 of them, add up exactly in float64 in any order
    assert np.array_equal(PJ.bits(s), PJ.bits(s_rev)) and np.array_equal(PJ.bits(s), PJ.bits(s_one))
    assert np.allclose(g, g_rev, rtol=1e-9, atol=1e-6) and np.allclose(g, g_one, rtol=1e-9, atol=1e-6)  # the same sums all the same


def test_order_sensitivity_of_the_column_sums_at_a_wider_span():
    """Magnitudes 2^-40 .. 2^20: now the column sums round as well, and their order shows."""
    x = PJ.mixed_magnitudes(lo=-40, hi=20, seed=1718)
    s, _ = PJ.moments(x)
    assert (PJ.bits(s) != PJ.bits(PJ.moments(x, reverse=True)[0])).any()
    assert (PJ.bits(s) != PJ.bits(PJ.moments(x, block=x.shape[0])[0])).any()


# ---- the fit ---------------------------------------------------------------------------------------------------------------------
N, D, R = 4000, 32, 4


@pytest.fixture(scope="module")
def planted():
    x, mean, basis, signal, eps = PJ.planted(N, D, R, seed=11, noise=0.01)
    return {"x": x, "mean": mean, "basis": basis, "signal": signal, "eps": eps, "sum": x.sum(axis=0), "gram": x.T @ x}


def _cov(a, b=None):
    b = a if b is None else b
    return (a - a.mean(axis=0)).T @ (b - b.mean(axis=0)) / a.shape[0]


@pytest.mark.parametrize("whiten", [False, True])
def test_fit_on_planted_data(planted, whiten):
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, R, whiten=whiten)
    assert p.mean.dtype == p.components.dtype == p.eigenvalues.dtype == np.float64
    assert p.components.shape == (R, D) and p.eigenvalues.shape == (D,) and p.n_rows == N and p.whiten is whiten and p.eps == 0.0
    assert np.allclose(p.mean, planted["x"].mean(axis=0), rtol=0, atol=1e-12)
    assert (np.diff(p.eigenvalues) <= 0).all()
    assert abs(p.explained_variance_ratio.sum() - 1.0) <= 1e-12 and p.explained_variance_ratio.shape == (D,)
    # W C W^T = diag(lambda), or I when whitened
    C = _cov(planted["x"])
    got = p.components @ C @ p.components.T
    want = np.eye(R) if whiten else np.diag(p.eigenvalues[:R])
    assert np.abs(got - want).max() <= 1e-9
    # the sign rule: the entry of largest magnitude of each eigenvector is positive, the lowest index among equals
    for row in p.components:
        assert row[np.argmax(np.abs(row))] > 0


def test_fitted_subspace_is_the_planted_one_within_davis_kahan(planted):
    """The sample covariance is A + H with A = cov(signal), whose range is the planted subspace U (rank R, smallest non-zero
    eigenvalue a_R, then 0), and H = cov(signal, noise) + cov(noise, signal) + cov(noise).  Davis-Kahan in the form of Yu, Wang
    and Samworth (Biometrika 2015, theorem 2): ||sin Theta(fitted, U)||_F <= 2 sqrt(R) ||H||_op / (a_R - 0), and every sine is
    at most that norm.  With noise 0.01 against a smallest planted variance of 1/8 the right-hand side is a few per cent
    (asserted below 0.1 from the planted pieces alone)."""
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, R)
    A = _cov(planted["signal"])
    H = _cov(planted["signal"], planted["eps"]) + _cov(planted["eps"], planted["signal"]) + _cov(planted["eps"])
    a = np.sort(np.linalg.eigvalsh(A))[::-1]
    assert a[R] <= 1e-12 * a[0]
    bound = 2.0 * math.sqrt(R) * np.linalg.norm(H, 2) / a[R - 1]
    assert bound < 0.1, bound
    cosines = np.linalg.svd(p.components @ planted["basis"].T, compute_uv=False)
    sines = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(cosines, 1.0) ** 2))
    print(f"largest principal-angle sine {sines.max():.3e}, Davis-Kahan bound {bound:.3e}")
    assert sines.max() <= bound


def test_sign_rule_takes_the_lowest_index_among_equal_magnitudes():
    """Two columns that are always equal: the leading eigenvector is (1, 1, 0) / sqrt 2 up to sign, a tie the rule breaks at index 0."""
    t = np.linspace(-1, 1, 9)
    x = np.stack([t, t, 0.1 * np.cos(7 * t)], axis=1)
    p = RC.projection_from_moments(x.sum(axis=0), x.T @ x, 9, 1)
    v = p.components[0]
    assert v[0] > 0 and abs(abs(v[0]) - abs(v[1])) < 1e-12


def test_eps_enters_the_whitening(planted):
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, 2, whiten=True, eps=0.25)
    q = RC.projection_from_moments(planted["sum"], planted["gram"], N, 2)
    assert np.allclose(p.components, q.components / np.sqrt(p.eigenvalues[:2] + 0.25)[:, None], rtol=1e-15, atol=0) and p.eps == 0.25


# ---- refusals: the field, the value, the supported set ---------------------------------------------------------------------------
def _small(n, d, seed=3):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x.sum(axis=0), x.T @ x


@pytest.mark.parametrize("n,d,m,says", [
    (100, 16, 0, ("n_components = 0", "1..d", "d = 16")),
    (100, 16, 17, ("n_components = 17", "1..d", "d = 16")),
    (10, 64, 32, ("n_components = 32", "1..9", "rank")),
    (1, 16, 4, ("n = 1", "at least 2")),
])
def test_refusals(n, d, m, says):
    s, g = _small(n, d)
    with pytest.raises(ValueError) as e:
        RC.projection_from_moments(s, g, n, m)
    for part in says:
        assert part in str(e.value), (part, str(e.value))


def test_transform_refuses_a_width_the_row_kernels_do_not_take(planted):
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, 2)
    with pytest.raises(ValueError, match=r"n_components = 2 .*multiple of 64"):
        p.transform([[0.0] * D])


# ---- the store -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whiten,suffix", [(False, ".npz"), (True, "")])
def test_projection_round_trip_is_bit_exact(planted, tmp_path, whiten, suffix):
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, 3, whiten=whiten, eps=1e-7 if whiten else 0.0)
    path = store.save_projection(p, str(tmp_path / "sub" / ("fit" + suffix)))
    assert path.endswith("fit.npz") and os.path.isfile(path) and os.listdir(tmp_path / "sub") == ["fit.npz"]
    q = store.load_projection(str(tmp_path / "sub" / ("fit" + suffix)))
    for f in ("mean", "components", "eigenvalues", "explained_variance_ratio"):
        a, b = getattr(p, f), getattr(q, f)
        assert b.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes(), f
    assert (q.n_rows, q.whiten, q.eps) == (p.n_rows, p.whiten, p.eps) and type(q.n_rows) is int and type(q.whiten) is bool


# ---- project_collection --------------------------------------------------------------------------------------------------------
def test_project_collection_keeps_ids_order_documents_and_metadatas(planted):
    p = RC.projection_from_moments(planted["sum"], planted["gram"], N, 3)
    col = RegionCollection(metric="sqeuclidean")
    ids = [f"r{7 * i % 10}" for i in range(10)]  # not sorted
    vecs = [planted["x"][i].astype(np.float32) for i in range(10)]
    vecs[4] = None  # a failed embedding stays a hole
    docs = [None if i == 2 else f"doc {i}" for i in range(10)]
    metas = [{"parent_image_name": f"page{i % 3}", "is_region": i != 0, "area_percentage": float(i)} for i in range(10)]
    col.upsert(ids=ids, embeddings=vecs, documents=docs, metadatas=metas)

    def host_transform(v):  # what Projection.transform computes, without the bf16 rounding and the device
        y = (np.asarray(v, dtype=np.float64) - p.mean) @ p.components.T
        return y / np.linalg.norm(y, axis=1, keepdims=True)

    before = col.get(include=["metadatas", "embeddings", "documents"])
    new = RC.project_collection(col, p, transform=host_transform)
    after = new.get(include=["metadatas", "embeddings", "documents"])
    assert after["ids"] == ids and after["documents"] == docs and after["metadatas"] == metas
    assert new.metric == "sqeuclidean" and new.count() == 10
    assert new.metadata["projection"] == {"n_components": 3, "whiten": False, "n_rows": N} and new.metadata["hnsw_space"] == "sqeuclidean"
    want = host_transform([v for v in vecs if v is not None])
    got = [e for e in after["embeddings"]]
    assert got[4] is None
    assert np.allclose(np.stack([e for e in got if e is not None]), want, rtol=0, atol=1e-6)
    # the source is unchanged
    again = col.get(include=["metadatas", "embeddings", "documents"])
    assert again["ids"] == before["ids"] and "projection" not in col.metadata
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(again["embeddings"], vecs))
