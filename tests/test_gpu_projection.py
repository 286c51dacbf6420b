"""K17 on the GPU (include/mme.h, mme_moments / mme_project): the moments bit for bit against the float64
restatement (tests/projection_reference.py), the projection against float64 within the derived bound on every element, the
L2 step bit for bit against mme_normalise_rows, the fit end to end on a planted table, and the refusals.

The planted inputs of the projection are built on the CPU first (case_inputs) and it is asserted there, before the GPU is asked,
that the same projection through bf16 weights would break the bound: a kernel that rounds the weights cannot pass."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_reference as PJ  # noqa: E402

pytestmark = pytest.mark.gpu

B = PJ.BLOCK


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    assert Engine.MOMENTS_BLOCK == B
    return Engine(0)


def _bf16(x64):
    """float64 numpy holding bf16 values -> bfloat16 CUDA tensor of exactly these values"""
    return torch.from_numpy(PJ.to_bf16_bits(x64).view(np.int16)).cuda().view(torch.bfloat16)


# ---- moments, bit for bit ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(n, d, seed):
    """any finite values, not unit rows: a common offset, columns of different scale"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) + 0.7) * rng.uniform(0.01, 30.0, d)
    return PJ.bf16_exact(x)


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name == "mixed":
        return PJ.mixed_magnitudes()
    if name == "wide":
        return PJ.mixed_magnitudes(lo=-40, hi=20, seed=1718)
    n, d = (int(v) for v in name.split("x"))
    return table(n, d, 100 + n % 97 + d)


@functools.lru_cache(maxsize=None)
def want_moments(name):
    s, g = PJ.moments(fixture(name))
    return PJ.bits(s), PJ.bits(g)


MOMENT_CASES = ["150x64", "150x128", "150x768", "150x1024", "1x64", f"{B - 1}x64", f"{B}x64", f"{B + 1}x64", f"{2 * B + 3}x64", "mixed", "wide"]


@pytest.mark.parametrize("name", MOMENT_CASES)
def test_moments_bit_for_bit(engine, name):
    x = _bf16(fixture(name))
    ws, wg = want_moments(name)
    s, g = engine.moments(x)
    s2, g2 = engine.moments(x)
    torch.cuda.synchronize()
    s, g, s2, g2 = (PJ.bits(t.cpu().numpy()) for t in (s, g, s2, g2))
    assert np.array_equal(g, g.T), "gram is not symmetric bit for bit"
    assert np.array_equal(s, s2) and np.array_equal(g, g2), "two runs differ"
    assert np.array_equal(s, ws), f"sum differs from the restatement in {int((s != ws).sum())} of {s.size} values"
    assert np.array_equal(g, wg), f"gram differs from the restatement in {int((g != wg).sum())} of {g.size} values"


@pytest.mark.parametrize("name,group", [(f"{2 * B + 3}x64", 1), (f"{2 * B + 3}x64", 2), ("mixed", 1), ("mixed", 3), ("wide", 2)])
def test_moments_in_block_groups_give_the_same_bits(engine, name, group):
    """the workspace forced short: `group` row blocks per launch, each group continuing where the one before stopped"""
    ws, wg = want_moments(name)
    s, g = engine.moments(_bf16(fixture(name)), group_blocks=group)
    s, g = PJ.bits(s.cpu().numpy()), PJ.bits(g.cpu().numpy())
    assert np.array_equal(s, ws) and np.array_equal(g, wg) and np.array_equal(g, g.T)


# ---- projection against float64 ---------------------------------------------------------------------------------------------------
SHAPES = [(64, 1), (64, 3), (64, 64), (128, 65), (768, 256), (1024, 1024)]
ROWS = [1, 63, 65, 257]


@functools.lru_cache(maxsize=None)
def case_inputs(d, m, n):
    """The cancellation case: unit rows 0.8 u + 0.6 v (u one direction shared by all rows, v a random unit vector), the mean
    0.8 u, and whitened weights: m orthonormal rows scaled to norms 1 .. 100 (100 alone when m == 1).
    -> x64 (bf16 values), mean32, w32, y64, bound"""
    rng = np.random.default_rng(1000 * d + 10 * m + n)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    v = rng.standard_normal((n, d))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    x64 = PJ.bf16_exact(0.8 * u + 0.6 * v)
    mean32 = (0.8 * u).astype(np.float32)
    q = np.linalg.qr(rng.standard_normal((d, m)))[0].T
    norms = np.array([100.0]) if m == 1 else np.logspace(0, 2, m)
    w32 = (q * norms[:, None]).astype(np.float32)
    y64, bound = PJ.project(x64, mean32, w32)
    return x64, mean32, w32, y64, bound


def through_bf16_weights(x64, mean32, w32):
    """what a bf16 GEMM would compute, its accumulation taken as exact: W_bf16 . x - W . mean"""
    return x64 @ PJ.bf16_exact(w32).T - mean32.astype(np.float64) @ w32.astype(np.float64).T


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d,m", SHAPES)
def test_projection_within_the_f32_bound(engine, d, m, n):
    x64, mean32, w32, y64, bound = case_inputs(d, m, n)
    assert np.abs(mean32.astype(np.float64)).max() < 0.8 and abs(np.linalg.norm(mean32.astype(np.float64)) - 0.8) < 1e-6
    assert abs(np.linalg.norm(w32.astype(np.float64), axis=1).max() - 100.0) < 1e-3
    # on the CPU, before the GPU is asked: bf16 weights would break the bound
    assert (np.abs(through_bf16_weights(x64, mean32, w32) - y64) > bound).any(), "the case does not tell bf16 weights from f32 ones"
    x, mu, w = _bf16(x64), torch.from_numpy(mean32).cuda(), torch.from_numpy(w32).cuda()
    first = None
    for ld in ((m + 3) // 4 * 4, (m + 4 + 3) // 4 * 4):
        buf = torch.full((n, ld), 777.0, dtype=torch.float32, device="cuda")
        y = engine.project(x, mu, w, normalise=False, out_f32=buf[:, :m])
        torch.cuda.synchronize()
        assert y.data_ptr() == buf.data_ptr()
        got = buf.cpu().numpy()
        assert (got[:, m:] == 777.0).all(), f"ld_y = {ld}: the padding columns were written"
        err = np.abs(got[:, :m].astype(np.float64) - y64)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"d {d} m {m} N {n} ld {ld}: max |y - y64| / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), (ld, worst, err[worst], bound[worst])
        first = got[:, :m].copy() if first is None else first
        assert first.tobytes() == got[:, :m].tobytes(), "the row pitch changed a bit"
    if m % 4 == 0:  # the tensor the engine allocates itself
        assert engine.project(x, mu, w, normalise=False).cpu().numpy().tobytes() == first.tobytes()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d,m", [s for s in SHAPES if s[1] % 64 == 0])
def test_normalised_rows_are_those_of_normalise_rows(engine, d, m, n):
    """y_bf16 == mme_normalise_rows(y_f32) bit for bit: both outputs of one call (dense rows: the row kernel reads the caller's;
    padded rows: it reads the workspace), and each output of a call of its own"""
    x64, mean32, w32, _, _ = case_inputs(d, m, n)
    x = _bf16(x64)
    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy()  # noqa: E731
    y32 = engine.project(x, mean32, w32, normalise=False)
    want = bits(engine.normalise_rows(y32.contiguous()))
    alone = engine.project(x, mean32, w32)
    both16, both32 = engine.project(x, mean32, w32, f32=True)
    pad = torch.full((n, m + 4), 777.0, dtype=torch.float32, device="cuda")
    pad16, pad32 = engine.project(x, mean32, w32, out_f32=pad[:, :m])
    torch.cuda.synchronize()
    assert alone.dtype == torch.bfloat16 and tuple(alone.shape) == (n, m)
    for name, got in (("bf16 alone", alone), ("both, dense", both16), ("both, padded", pad16)):
        assert np.array_equal(bits(got), want), name
    for name, got in (("both, dense", both32), ("both, padded", pad32)):
        assert torch.equal(got, y32), name
    assert (pad[:, m:] == 777.0).all()
    norms = np.linalg.norm(alone.float().cpu().numpy().astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 2.0 ** -7


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_table():
    """N = 600, d = 128: a common component, a planted rank-8 part, noise; -> float32 rows (not unit: the library normalises)"""
    x, mean, basis, _, _ = PJ.planted(600, 128, 8, seed=23, noise=0.01, mean_scale=2.0)
    return x.astype(np.float32), basis


def test_fit_whiten_transform_gives_identity_covariance(engine):
    """The whitened coordinates of the fitted rows have covariance I.  The tolerance: with y = y* + e (y* the float64 projection with
    the float64 mean and weights, whose covariance is I to 1e-9 by the fit), cov(y) - I = cov(y*, e) + cov(e, y*) + cov(e), and
    |cov(y*_j, e_k)| <= sd(y*_j) max_i |e_ik| = E_k; so |cov(y) - I|_jk <= E_j + E_k + E_j E_k + 1e-9.  E_k is the f32 bound of the
    kernel plus what the one rounding of mean and weights to f32 moves y64 by: 2^-24 (sum_c |mean| |w| + sum_c |x - mean| |w|)."""
    from multimodal_embeddings_amd import region_compare as RC
    from multimodal_embeddings_amd.cross_compare import to_unit_bf16

    x32, _ = planted_table()
    p = RC.fit_projection(x32, 8, whiten=True, engine=engine)
    assert p.n_rows == 600 and p.components.shape == (8, 128) and p.whiten
    rows = to_unit_bf16(x32, engine)
    x64 = rows.float().cpu().numpy().astype(np.float64)
    # the fit is the host half on the device's moments, and those are the restatement's
    s, g = PJ.moments(x64)
    q = RC.projection_from_moments(s, g, 600, 8, whiten=True)
    assert q.components.tobytes() == p.components.tobytes() and q.mean.tobytes() == p.mean.tobytes()
    y = p.transform(x32, normalise=False, engine=engine)
    assert y.dtype == torch.float32 and tuple(y.shape) == (600, 8)
    y = y.cpu().numpy().astype(np.float64)
    mean32, w32 = p.mean.astype(np.float32), p.components.astype(np.float32)
    y64, bound = PJ.project(x64, mean32, w32)
    assert (np.abs(y - y64) <= bound).all()
    cen, aw = np.abs(x64 - p.mean), np.abs(p.components)
    E = (bound + 2.0 ** -24 * 1.01 * (np.abs(p.mean) @ aw.T + cen @ aw.T)).max(axis=0)
    tol = E[:, None] + E[None, :] + E[:, None] * E[None, :] + 1e-9
    cov = np.cov(y.T, bias=True)
    print(f"max |cov - I| = {np.abs(cov - np.eye(8)).max():.3e}, smallest tolerance {tol.min():.3e}")
    assert (np.abs(cov - np.eye(8)) <= tol).all()


def test_projected_collection_feeds_cosine_and_clustering(engine):
    from multimodal_embeddings_amd import region_compare as RC
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    x32, _ = planted_table()
    col = RegionCollection(engine=engine)
    ids = [f"reg{i:04d}" for i in range(600)]
    metas = [{"parent_image_name": f"page{i % 7}.jpg", "region_type": "text", "area_percentage": 1.0 + i % 5, "is_region": True} for i in range(600)]
    col.upsert(ids=ids, embeddings=[v for v in x32], documents=[f"d{i}" for i in range(600)], metadatas=metas)
    p = RC.fit_projection(col, 64, engine=engine)
    assert p.n_components == 64 and p.n_rows == 600
    new = RC.project_collection(col, p, engine=engine)
    got = new.get(include=["metadatas", "embeddings", "documents"])
    assert got["ids"] == ids and got["metadatas"] == metas and got["documents"] == [f"d{i}" for i in range(600)]
    assert new.metadata["projection"] == {"n_components": 64, "whiten": False, "n_rows": 600}
    emb = np.stack(got["embeddings"])
    assert emb.shape == (600, 64) and np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1.0).max() < 2.0 ** -7
    rows = p.transform(x32, engine=engine)
    S = engine.cosine(rows)
    torch.cuda.synchronize()
    assert tuple(S.shape) == (600, 600) and float((S.diagonal() - 1.0).abs().max()) < 0.02
    out = RC.cluster_regions(new, 4, engine=engine)
    assert out["n_regions"] == 600 and out["n_clusters"] == 4 and sum(c["size"] for c in out["clusters"]) == 600


def test_a_text_shaped_query_ranks_its_planted_neighbour_first(engine):
    """A query vector that is no row of the table (a list of floats, as a text tower hands it over): row 123 plus a small
    perturbation.  After the same transform its cosine with the projected row 123 is the largest of all 600."""
    from multimodal_embeddings_amd import region_compare as RC

    x32, _ = planted_table()
    p = RC.fit_projection(x32, 64, whiten=True, eps=1e-6, engine=engine)
    rows = p.transform(x32, engine=engine)
    rng = np.random.default_rng(77)
    query = (x32[123] + 0.002 * rng.standard_normal(128)).astype(np.float32)
    q = p.transform([query.tolist()], engine=engine)
    assert q.dtype == torch.bfloat16 and tuple(q.shape) == (1, 64)
    S = engine.cosine(q, rows).cpu().numpy()[0]
    assert int(np.argmax(S)) == 123, (int(np.argmax(S)), float(S.max()), float(S[123]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_context_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError

    name = f"{B + 1}x64"
    x = _bf16(fixture(name))
    n, d = x.shape
    ws, wg = want_moments(name)
    x64, mean32, w32, y64, bound = case_inputs(64, 64, 65)
    px, mu, w = _bf16(x64), torch.from_numpy(mean32).cuda(), torch.from_numpy(w32).cuda()
    fill = -7.5e300
    s = torch.full((d,), fill, dtype=torch.float64, device="cuda")
    g = torch.full((d, d), fill, dtype=torch.float64, device="cuda")
    y32 = torch.full((65, 68), 777.0, dtype=torch.float32, device="cuda")
    y16 = torch.full((65, 64), 3.0, dtype=torch.bfloat16, device="cuda")
    lib, h = engine.lib, engine.h

    def moments(emb=x.data_ptr(), N=n, dd=d, sp=s.data_ptr(), gp=g.data_ptr(), apply_group=None):
        if apply_group is None:
            rc = lib.mme_moments(h, emb, N, dd, sp, gp, engine._stream())
        else:
            rc = lib.mme_moments_apply(h, emb, N, dd, apply_group, sp, gp, engine._stream())
        return rc, lib.mme_last_error(h).decode()

    def project(emb=px.data_ptr(), N=65, dd=64, mp=mu.data_ptr(), wp=w.data_ptr(), m=64, f=y32.data_ptr(), ld=68, b=y16.data_ptr()):
        return lib.mme_project(h, emb, N, dd, mp, wp, m, f, ld, b, engine._stream()), lib.mme_last_error(h).decode()

    def untouched():
        torch.cuda.synchronize()
        return bool((s == fill).all() and (g == fill).all() and (y32 == 777.0).all() and (y16 == 3.0).all())

    def still_serves():
        s2, g2 = engine.moments(x)
        y = engine.project(px, mu, w, normalise=False)
        return (np.array_equal(PJ.bits(s2.cpu().numpy()), ws) and np.array_equal(PJ.bits(g2.cpu().numpy()), wg)
                and bool((np.abs(y.cpu().numpy().astype(np.float64) - y64) <= bound).all()))

    m_cases = [(dict(N=0), "N = 0"), (dict(N=(1 << 24) + 1), f"N = {(1 << 24) + 1}"), (dict(dd=32), "d = 32"), (dict(dd=96), "d = 96"),
               (dict(dd=1088), "d = 1088"), (dict(emb=None), "emb"), (dict(sp=None), "sum"), (dict(gp=None), "gram"),
               (dict(emb=x.data_ptr() + 2), "emb"), (dict(sp=s.data_ptr() + 4), "sum"), (dict(gp=g.data_ptr() + 4), "gram"),
               (dict(apply_group=-1), "group_blocks = -1"), (dict(apply_group=65536), "group_blocks = 65536")]
    for kw, text in m_cases:
        rc, msg = moments(**kw)
        assert rc == -1 and "mme_moments" in msg and text in msg and ("supported" in msg or "required" in msg), (kw, rc, msg)
        assert untouched(), kw
        assert still_serves(), kw
    p_cases = [(dict(N=0), "N = 0"), (dict(N=(1 << 24) + 1), f"N = {(1 << 24) + 1}"), (dict(dd=32), "d = 32"), (dict(dd=100), "d = 100"),
               (dict(m=0), "m = 0"), (dict(m=65), "m = 65"), (dict(m=32), "m = 32 with y_bf16"), (dict(f=None, b=None), "both null"),
               (dict(ld=60), "ld_y = 60"), (dict(ld=66), "ld_y = 66"), (dict(emb=None), "emb"), (dict(mp=None), "mean"), (dict(wp=None), "w ="),
               (dict(emb=px.data_ptr() + 2), "emb"), (dict(mp=mu.data_ptr() + 4), "mean"), (dict(wp=w.data_ptr() + 8), "w ="),
               (dict(f=y32.data_ptr() + 4), "y_f32"), (dict(b=y16.data_ptr() + 2), "y_bf16")]
    for kw, text in p_cases:
        rc, msg = project(**kw)
        assert rc == -1 and "mme_project" in msg and text in msg, (kw, rc, msg)
        assert untouched(), kw
        assert still_serves(), kw
    # the Python layer: its own checks, then the library's through MmeError
    with pytest.raises(MmeError, match="2-D bfloat16"):
        engine.moments(x.float())
    with pytest.raises(MmeError, match="d = 32"):
        engine.moments(x[:, :32])
    with pytest.raises(MmeError, match=r"mean must be \[d = 64\]"):
        engine.project(px, mean32[:32], w32)
    with pytest.raises(MmeError, match="m = 3 with y_bf16"):
        engine.project(px, mean32, w32[:3])
    with pytest.raises(MmeError, match="float32"):
        engine.project(px, mu.double(), w)
