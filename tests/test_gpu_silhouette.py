"""K16 on the GPU (include/mme.h, mme_silhouette): the samples bit for bit on inputs whose dot products are exact, planted
partitions against the float64 restatement (tests/silhouette_reference.py) within the f64 dot-product bound, the edges, the
refusals, and choosing the number of clusters through region_compare on a committed fixture whose margins are asserted first."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_reference as K  # noqa: E402
import silhouette_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel elements in front of and behind every output
U = 2.0 ** -53


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    return Engine(0)


class Guarded:
    """an output tensor between two runs of sentinels"""

    PATTERN = {torch.int32: -123456789, torch.float64: -7.5e300, torch.int64: -1234567890123}

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.fill = self.PATTERN[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD : GUARD + n].view(*shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[-GUARD:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


FIELDS = ("sample", "cluster", "score", "info", "sums", "counts")


def _buffers(N, d, k):
    return {"sample": Guarded((N,), torch.float64), "cluster": Guarded((k,), torch.float64), "score": Guarded((1,), torch.float64),
            "info": Guarded((2,), torch.int64), "sums": Guarded((k, d), torch.float64), "counts": Guarded((k,), torch.int32)}


def _call(engine, x, N, d, lab, k, bufs, null=(), out=True):
    from multimodal_embeddings_amd._lib import _SilhouetteOut

    o = _SilhouetteOut()
    for f in FIELDS:
        setattr(o, f, None if f in null else bufs[f].t.data_ptr())
    rc = engine.lib.mme_silhouette(engine.h, None if x is None else x.data_ptr(), N, d, None if lab is None else lab.data_ptr(), k,
                                   C.byref(o) if out else None, engine._stream())
    return rc, engine.lib.mme_last_error(engine.h).decode()


def _run_raw(engine, xb, labels, k, sample=True):
    """mme_silhouette on guarded buffers -> dict of numpy outputs (sentinels checked); the labels must come back unchanged"""
    N, d = xb.shape
    x = _bf16(xb)
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    bufs = _buffers(N, d, k)
    rc, msg = _call(engine, x, N, d, lab, k, bufs, null=() if sample else ("sample",))
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(g.intact() for g in bufs.values())
    assert sample or bufs["sample"].untouched()
    assert np.array_equal(lab.cpu().numpy(), labels) and np.array_equal(_bits(x), xb)
    return {f: g.t.cpu().numpy() for f, g in bufs.items()}


def _same_bits(a, b, fields=FIELDS):
    return all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in fields)


def _against(got, ref, N, d, *, exact=False):
    """the outputs against the restatement: samples within the dot-product bound (bit for bit when exact), the means with
    N 2^-53 more for the order of their adds, the integers and the NaN pattern exactly"""
    bound, least = (0.0, None) if exact else S.sample_bound(ref, d)
    assert got["info"].tolist() == ref["info"].tolist()
    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["sums"], ref["sums"])  # the update's adds in its order
    assert np.array_equal(np.isnan(got["sample"]), np.isnan(ref["sample"])) and np.array_equal(np.isnan(got["cluster"]), np.isnan(ref["cluster"]))
    ok = ~np.isnan(ref["sample"])
    err = float(np.abs(got["sample"][ok] - ref["sample"][ok]).max()) if ok.any() else 0.0
    print(f"N={N} d={d} k={len(ref['counts'])} sample err {err:.3e} bound {bound:.3e} least max(a, b) {least}")
    if exact:
        assert np.array_equal(got["sample"].view(np.uint64), ref["sample"].view(np.uint64)), np.argwhere(got["sample"].view(np.uint64) != ref["sample"].view(np.uint64))[:5].ravel()
    else:
        assert err <= bound, (err, bound)
    used = ~np.isnan(ref["cluster"])
    cerr = float(np.abs(got["cluster"][used] - ref["cluster"][used]).max()) if used.any() else 0.0
    assert cerr <= bound + N * U, (cerr, bound)
    if np.isnan(ref["score"]):
        assert np.isnan(got["score"][0])
    else:
        assert abs(got["score"][0] - ref["score"]) <= bound + N * U, (got["score"][0], ref["score"], bound)


# ---- the exact case ---------------------------------------------------------------------------------------------------

EXACT_SIZES = {(2, 2): [1, 1], (63, 2): [32, 31], (63, 3): [32, 16, 15], (257, 2): [256, 1], (257, 3): [128, 128, 1], (257, 65): [4] * 64 + [1]}


@pytest.mark.parametrize("N,k", sorted(EXACT_SIZES))
def test_samples_are_exact_on_signed_basis_vectors(engine, N, k):
    """rows +-e_t: every product is 0 or +-1, so g, q and the sums are integers whatever the order of the adds, and the samples
    are the restatement's operations on the same numbers"""
    d = 64
    sizes = EXACT_SIZES[(N, k)]
    assert sum(sizes) == N and len(sizes) == k
    rng = np.random.default_rng(N * 131 + k)
    lab = np.repeat(np.arange(k), sizes)[rng.permutation(N)].astype(np.int32)
    xb = np.zeros((N, d), dtype=np.uint16)
    # a cluster leans on a few axes of its own, so that the samples are not all alike
    axis = (lab * 7 + rng.integers(0, 3, N) * (rng.random(N) < 0.8) + rng.integers(0, d, N) * (rng.random(N) < 0.2)) % d
    xb[np.arange(N), axis] = np.where(rng.random(N) < 0.25, 0xBF80, 0x3F80)  # -1.0 / +1.0
    ref = S.by_sums(xb, lab, k)
    x64 = K.bf16_to_f64(xb)
    assert np.array_equal(ref["sums"], np.round(ref["sums"])) and np.array_equal(x64 @ ref["sums"].T, np.round(x64 @ ref["sums"].T))
    if N > 2:
        assert len(np.unique(ref["sample"])) > 3
    got = _run_raw(engine, xb, lab, k)
    _against(got, ref, N, d, exact=True)


# ---- planted partitions against the restatement ----------------------------------------------------------------------

KS = [2, 3, 63, 64, 65, 257, 1000]


@functools.lru_cache(maxsize=None)
def _planted(N, d, k):
    xb, lab = S.planted(N, d, k, seed=N * 7919 + d * 31 + k)
    ref = S.by_sums(xb, lab, k)
    bound, least = S.sample_bound(ref, d)
    assert least >= 1e-2, least  # the quotient's denominator: the bound means something
    assert ref["info"].tolist() == [N, k]
    return xb, lab, ref


@pytest.mark.parametrize("d", [64, 384, 768, 1024])
@pytest.mark.parametrize("N", [63, 257, 1031])
def test_planted_partitions_against_float64(engine, N, d):
    for k in KS:
        if k > N:
            continue
        xb, lab, ref = _planted(N, d, k)
        got = _run_raw(engine, xb, lab, k)
        _against(got, ref, N, d)


def test_two_calls_and_a_call_without_samples_give_the_same_bits(engine):
    for N, d, k in ((257, 64, 3), (1031, 384, 65), (1031, 768, 1000)):
        xb, lab, _ = _planted(N, d, k)
        first = _run_raw(engine, xb, lab, k)
        assert _same_bits(first, _run_raw(engine, xb, lab, k))
        without = _run_raw(engine, xb, lab, k, sample=False)  # sample = NULL
        assert _same_bits(first, without, fields=("cluster", "score", "info", "sums", "counts"))


def test_sums_and_counts_are_the_updates(engine):
    for N, d, k in ((257, 64, 3), (1031, 384, 65)):
        xb, lab, _ = _planted(N, d, k)
        lab = lab.copy()
        lab[[1, N - 2]] = [-1, k]  # rows of no cluster
        got = _run_raw(engine, xb, lab, k)
        sums, counts = torch.zeros((k, d), dtype=torch.float64, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda")
        cen = torch.zeros((k, d), dtype=torch.bfloat16, device="cuda")
        engine.kmeans_apply("update", emb=_bf16(xb), labels=torch.from_numpy(lab).cuda(), centroids=cen, sums=sums, counts=counts)
        assert np.array_equal(got["sums"].view(np.uint64), sums.cpu().numpy().view(np.uint64)) and np.array_equal(got["counts"], counts.cpu().numpy())


# ---- the edges ----------------------------------------------------------------------------------------------------------

def test_planted_edges(engine):
    N, d = 257, 64
    xb, base, _ = _planted(N, d, 3)
    # cluster 0 and cluster k - 1 empty: never a candidate for b, NaN means, not counted among the clusters with members
    k = 5
    lab = base + 1
    ref = S.by_sums(xb, lab, k)
    assert ref["counts"][0] == 0 and ref["counts"][4] == 0
    got = _run_raw(engine, xb, lab, k)
    _against(got, ref, N, d)
    assert np.isnan(got["cluster"][[0, 4]]).all() and got["info"].tolist() == [N, 3] and np.isfinite(got["sample"]).all()
    # a singleton gives exactly 0.0; a cluster of two bit-equal rows; rows of no cluster (labels -1 and k)
    k = 6
    lab = base.copy()
    xb2 = xb.copy()
    lab[10] = 3
    xb2[21] = xb2[20]
    lab[[20, 21]] = 4
    lab[[30, 31]] = [-1, k]
    ref = S.by_sums(xb2, lab, k)
    got = _run_raw(engine, xb2, lab, k)
    _against(got, ref, N, d)
    assert got["sample"][10] == 0.0 and not np.signbit(got["sample"][10]) and got["cluster"][3] == 0.0
    assert got["sample"][20] == got["sample"][21] and got["sample"][20] > 0.9  # their distance is 1 - q, next to nothing
    assert np.isnan(got["sample"][[30, 31]]).all() and got["info"].tolist() == [N - 2, 5] and np.isnan(got["cluster"][5])
    keep = np.ones(N, dtype=bool)
    keep[[30, 31]] = False
    alone = _run_raw(engine, xb2[keep], lab[keep], k)  # a row of no cluster is a member of nothing: leaving it out changes no bit
    assert np.array_equal(got["sample"][keep].view(np.uint64), alone["sample"].view(np.uint64)) and _same_bits(got, alone, fields=("cluster", "score", "sums", "counts"))
    # all rows but one in one cluster
    lab = np.zeros(N, dtype=np.int32)
    lab[100] = 1
    ref = S.by_sums(xb, lab, 2)
    got = _run_raw(engine, xb, lab, 2)
    _against(got, ref, N, d)
    assert got["sample"][100] == 0.0 and got["info"].tolist() == [N, 2] and got["counts"].tolist() == [N - 1, 1]
    # one cluster with members: no score
    lab = np.ones(N, dtype=np.int32)
    got = _run_raw(engine, xb, lab, 2)
    assert np.isnan(got["score"][0]) and got["info"].tolist() == [N, 1] and np.isnan(got["cluster"][0]) and got["cluster"][1] == 0.0
    assert not got["sample"].any()
    got = _run_raw(engine, xb, np.full(N, -1, dtype=np.int32), 2)  # and none at all
    assert np.isnan(got["score"][0]) and got["info"].tolist() == [0, 0] and np.isnan(got["sample"]).all() and np.isnan(got["cluster"]).all()


def test_the_engine_method_and_the_rows_kernel_alone(engine):
    from multimodal_embeddings_amd._lib import MmeError

    N, d, k = 1031, 384, 65
    xb, lab, ref = _planted(N, d, k)
    raw = _run_raw(engine, xb, lab, k)
    x, labels = _bf16(xb), torch.from_numpy(lab).cuda()
    res = engine.silhouette(x, labels, k, samples=True)
    assert res.score.item() == raw["score"][0] and np.array_equal(res.samples.cpu().numpy().view(np.uint64), raw["sample"].view(np.uint64))
    assert np.array_equal(res.cluster.cpu().numpy(), raw["cluster"]) and res.info.tolist() == [N, k] and np.array_equal(res.counts.cpu().numpy(), raw["counts"])
    assert engine.silhouette(x, labels, k).samples is None
    sample = Guarded((N,), torch.float64)
    engine.silhouette_rows(x, labels, res.sums, res.counts, sample.t)
    torch.cuda.synchronize()
    assert sample.intact() and np.array_equal(sample.t.cpu().numpy().view(np.uint64), raw["sample"].view(np.uint64))
    for kw, text in [(dict(emb=x.float()), "2-D bfloat16"), (dict(labels=labels.long()), "int32 tensor"), (dict(labels=labels[:-1]), "int32 tensor"),
                     (dict(k=1), "k = 1"), (dict(k=N + 1), f"k = {N + 1}")]:
        args = dict(emb=x, labels=labels, k=k)
        args.update(kw)
        with pytest.raises(MmeError) as e:
            engine.silhouette(args["emb"], args["labels"], args["k"])
        assert text in str(e.value), (kw, str(e.value))


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_name_the_field_and_leave_the_context_usable(engine):
    N, d, k = 257, 64, 3
    xb, lab_np, _ = _planted(N, d, k)
    good = _run_raw(engine, xb, lab_np, k)
    x, lab = _bf16(xb), torch.from_numpy(lab_np).cuda()
    narrow = _bf16(xb[:, :32].copy())
    bufs = _buffers(N, d, k)

    def call(emb=x, n=N, dd=d, labels=lab, kk=k, null=(), out=True):
        return _call(engine, emb, n, dd, labels, kk, bufs, null=null, out=out)

    cases = [(dict(n=1), "N = 1"), (dict(n=0), "N = 0"), (dict(emb=narrow, dd=32), "d = 32"), (dict(dd=0), "d = 0"), (dict(kk=1), "k = 1"), (dict(kk=0), "k = 0"),
             (dict(kk=N + 1), f"k = {N + 1} is outside 2..min(N, 65536) (N = {N})"), (dict(n=70000, kk=65537), "k = 65537"), (dict(emb=None), "emb is null"),
             (dict(labels=None), "labels is null"), (dict(out=False), "out is null")]
    cases += [(dict(null=(f,)), f"out.{f} is null") for f in FIELDS if f != "sample"]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and "mme_silhouette" in msg and text in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in bufs.values()), kw  # nothing was enqueued
        assert _same_bits(good, _run_raw(engine, xb, lab_np, k))  # and the context serves the next call
    rc, msg = call(null=("sample",))  # the one pointer that may be null
    assert rc == 0, msg


# ---- choosing k through region_compare ----------------------------------------------------------------------------------------

def _collection(x32):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    col = RegionCollection()
    n = len(x32)
    ids = [f"region_{r}" for r in range(n)]
    metas = [{"parent_image": f"/data/pages/page{r % 7}.png", "region_type": "advert", "area_percentage": 2.0, "is_region": True} for r in range(n)]
    col.upsert(ids=ids, embeddings=x32.tolist(), metadatas=metas)
    col.upsert(ids=["page_0"], embeddings=[x32[0].tolist()], metadatas=[{"parent_image": "/data/pages/page0.png", "is_region": False}])
    return col, ids


def test_choosing_k_is_the_restatements_choice(engine):
    from multimodal_embeddings_amd import region_compare as rc
    from multimodal_embeddings_amd.cross_compare import to_unit_bf16

    g = np.load(os.path.join(S.GOLDEN, "silhouette_choose.npz"))
    c = S.CHOOSE
    x32, seed = g["x"], int(g["seed"])
    n, d = x32.shape
    col, ids = _collection(x32)
    bits = _bits(to_unit_bf16(x32.tolist(), engine))  # the rows as the collection's loader makes them
    runs, picked = S.choose_k(bits, c["k_range"], seed, c["max_iter"])
    # on the restatement alone: no label hangs on the GEMM's rounding, and the choice not on the silhouette's
    assert all(v["run"]["gap"] > 4 * K.delta(d) and v["run"]["converged"] for v in runs.values()), {k: v["run"]["gap"] / K.delta(d) for k, v in runs.items()}
    scores = sorted((v["sil"]["score"] for v in runs.values()), reverse=True)
    assert scores[0] - scores[1] > 1e-6
    table, arr = rc.kmeans_regions(col, n_clusters=None, k_range=c["k_range"], init="random", seed=seed, max_iter=c["max_iter"], engine=engine,
                                   silhouette_samples=True)
    assert sorted(table["k_scores"]) == sorted(arr["by_k"]) == list(c["k_range"])
    for k, v in runs.items():
        assert np.array_equal(arr["by_k"][k]["labels"], v["run"]["labels"]), k
        bound, least = S.sample_bound(v["sil"], d)
        assert least >= 1e-2 and abs(table["k_scores"][k] - v["sil"]["score"]) <= bound + n * U, (k, table["k_scores"][k], v["sil"]["score"])
    assert picked == int(g["picked"]) == c["centres"] and table["n_clusters"] == picked and rc.pick_n_clusters(table["k_scores"]) == picked
    ref = runs[picked]
    bound, _ = S.sample_bound(ref["sil"], d)
    assert table["silhouette"] == table["k_scores"][picked] and np.array_equal(arr["labels"], ref["run"]["labels"])
    assert table["iterations"] == ref["run"]["iterations"] and table["converged"] is True and table["n_empty"] == 0
    assert float(np.abs(arr["silhouette_samples"] - ref["sil"]["sample"]).max()) <= bound
    want = rc.cluster_table(ref["run"]["labels"], arr["sim"], ids, [m for m in col.get(where={"is_region": {"$eq": True}})["metadatas"]], n_clusters=picked)
    for cl, w, s in zip(table["clusters"], want["clusters"], ref["sil"]["cluster"]):
        assert cl["size"] == w["size"] and [m["id"] for m in cl["members"]] == [m["id"] for m in w["members"]] and cl["medoid"] == w["medoid"]
        assert abs(cl["silhouette"] - s) <= bound + n * U
    # the same k asked for by name is the same table; the new keys only on request
    named, arr2 = rc.kmeans_regions(col, picked, init="random", seed=seed, max_iter=c["max_iter"], engine=engine, silhouette=True)
    assert named["k_scores"] == {picked: table["silhouette"]} and named["silhouette"] == table["silhouette"] and "by_k" not in arr2 and "silhouette_samples" not in arr2
    assert named["clusters"] == table["clusters"]
    # labels the caller already has
    scored = rc.silhouette_regions(col, arr["labels"], engine=engine)
    assert scored["silhouette"] == table["silhouette"] and scored["n_clusters"] == picked and scored["n_regions"] == n
    assert [cl["silhouette"] for cl in scored["clusters"]] == [cl["silhouette"] for cl in table["clusters"]]
    assert np.array_equal(np.array(scored["samples"]), arr["silhouette_samples"])
    with pytest.raises(ValueError, match="1 cluster"):
        rc.silhouette_regions(col, np.zeros(n, dtype=np.int32), engine=engine)
    report = rc.create_region_cluster_report(col, None, k_range=range(3, 6), init="random", seed=seed, engine=engine)
    assert sorted(report["k_scores"]) == [3, 4, 5] and report["n_clusters"] == picked


def test_without_the_new_keywords_the_output_is_todays(engine):
    from multimodal_embeddings_amd import region_compare as rc

    g = np.load(os.path.join(S.GOLDEN, "silhouette_choose.npz"))
    col, ids = _collection(g["x"][:120])
    table = rc.cluster_regions(col, 4, engine=engine)
    assert set(table) == {"n_regions", "n_clusters", "n_empty", "iterations", "converged", "objective", "clusters"}
    assert all(set(cl) == {"cluster", "size", "cohesion", "medoid", "pages", "members"} for cl in table["clusters"])
    t2, arr = rc.kmeans_regions(col, 4, engine=engine)
    assert t2 == table and set(arr) == {"ids", "labels", "sim", "centroids", "counts", "objectives", "best_run"}
    t3 = rc.cluster_regions(col, 4, engine=engine, silhouette=True)
    assert set(t3) - set(table) == {"k_scores", "silhouette"} and all(set(a) - set(b) == {"silhouette"} for a, b in zip(t3["clusters"], table["clusters"]))
    assert {k: v for k, v in t3.items() if k in table and k != "clusters"} == {k: v for k, v in table.items() if k != "clusters"}
