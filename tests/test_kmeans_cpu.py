"""K15 (spherical k-means) without a GPU: the exports, the float64 restatement on a hand-made case, the report table, the
start forms, the Python-side refusals, and the condition the whole-run GPU cases rely on (tests/kmeans_reference.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_reference as R  # noqa: E402

from multimodal_embeddings_amd import region_compare as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_exports_carry_kmeans():
    from multimodal_embeddings_amd import _lib, build

    with open(os.path.join(ROOT, "include", "mme.h")) as fh:
        header = fh.read()
    for name in ("mme_kmeans", "mme_kmeans_apply"):
        assert re.search(r"\bint %s\(mme_ctx\*" % name, header), name
        assert name in _lib.EXPORTS
    assert "#define MME_ABI_VERSION 2" in header
    # the struct mirrors have the header's fields, in its order
    body = re.search(r"typedef struct mme_kmeans_state \{(.*?)\} mme_kmeans_state;", header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in _lib._KmeansState._fields_]
    body = re.search(r"typedef struct mme_kmeans_apply_args \{(.*?)\} mme_kmeans_apply_args;", header, re.S).group(1)
    names = [n for decl in re.findall(r"^\s*[^/\n]*?([\w, *]+);", body, re.M) for n in re.findall(r"(\w+)\s*(?:,|$)", decl)]
    assert names == [f for f, _ in _lib._KmeansApplyArgs._fields_]
    assert "kmeans.hip" in build.SOURCES and "capi_kmeans.hip" in build.SOURCES and "kmeans.h" in build.HEADERS


def test_bf16_rounding_is_one_rounding_to_nearest_even():
    one = float(R.bf16_to_f64(np.uint16(0x3F80)))
    ulp = 2.0 ** -7
    cases = [(1.0, 0x3F80), (1.0 + ulp / 2, 0x3F80), (1.0 + 3 * ulp / 2, 0x3F82), (1.0 + ulp / 2 + 2.0 ** -40, 0x3F81),
             (-(1.0 + ulp / 2), 0xBF80), (0.0, 0x0000), (-0.0, 0x8000), (1.0 - ulp / 4, 0x3F80), (1.0 - 3 * ulp / 8, 0x3F7F),
             # f32 would round this down to the tie 1 + ulp / 2 first, and the tie then to even 1.0: one rounding gives 1 + ulp
             (1.0 + ulp / 2 + 2.0 ** -30, 0x3F81)]
    assert one == 1.0
    for x, want in cases:
        assert int(R.f64_to_bf16(np.float64(x))) == want, (x, hex(int(R.f64_to_bf16(np.float64(x)))), hex(want))
    v = np.random.default_rng(0).standard_normal(4096)
    back = R.bf16_to_f64(R.f64_to_bf16(v))
    assert np.all(np.abs(back - v) <= np.abs(v) * 2.0 ** -8) and np.array_equal(R.f64_to_bf16(back), R.f64_to_bf16(v))


def _six_points():
    """6 unit rows in d = 64 around two axes: rows 0..2 near e0, rows 3..5 near e1; every value is exact in bf16"""
    x = np.zeros((6, 64))
    x[0, 0], x[1, :2], x[2, [0, 2]] = 1.0, (0.96875, 0.25), (0.96875, 0.25)
    x[3, 1], x[4, [1, 0]], x[5, [1, 3]] = 1.0, (0.96875, 0.25), (0.96875, 0.25)
    bits = R.f64_to_bf16(x)
    assert np.array_equal(R.bf16_to_f64(bits), x)
    return bits


def test_reference_on_six_points():
    bits = _six_points()
    # start on rows 0 and 1, both of the first group: the first assignment splits group one and puts group two with row 1
    ref = R.run(bits, bits[[0, 1]], 10)
    assert ref["labels"].tolist() == [0, 0, 0, 1, 1, 1] and ref["counts"].tolist() == [3, 3]
    assert ref["converged"] and ref["iterations"] == 2 and ref["moved"] == 0 and ref["empty"] == 0
    first = R.run(bits, bits[[0, 1]], 0)
    assert first["labels"].tolist() == [0, 1, 0, 1, 1, 1] and first["iterations"] == 0 and not first["converged"]
    assert np.array_equal(first["centroids"], bits[[0, 1]]) and not first["sums"].any()
    assert first["sim"].tolist() == [1.0, 0.96875 ** 2 + 0.25 ** 2, 0.96875, 0.25, 2 * 0.96875 * 0.25, 0.96875 * 0.25]
    one = R.run(bits, bits[[0, 1]], 1)
    assert one["iterations"] == 1 and not one["converged"] and one["moved"] == 1 and one["counts"].tolist() == [2, 4]
    assert one["sums"][0, :3].tolist() == [1.96875, 0.0, 0.25] and one["sums"][1, :4].tolist() == [1.21875, 3.1875, 0.0, 0.25]
    # the centroid is the f64 mean direction, rounded once; the labels describe the returned centroids
    x64 = R.bf16_to_f64(bits)
    s = x64[:3].sum(axis=0)
    assert np.array_equal(ref["centroids"][0], R.f64_to_bf16(s / np.sqrt((s * s).sum())))
    lab, sim, _ = R.assign(x64, R.bf16_to_f64(ref["centroids"]))
    assert np.array_equal(lab, ref["labels"]) and np.array_equal(sim, ref["sim"]) and ref["objective"] == sim.sum()
    assert 0.03 < ref["gap"] < 0.031  # row 0 in the first assignment: itself against row 1
    # two equal start rows: every tie goes to the lower cluster; in the first update the second is empty and keeps its row
    # (which then draws the rows of its own blob, nearer to it than to the mean of all)
    both = np.concatenate([bits, bits[:1]])
    dup = R.run(both, both[[0, 6]], 1)
    assert dup["counts"].tolist() == [7, 0] and dup["empty"] == 1 and np.array_equal(dup["centroids"][1], bits[0]) and not dup["sums"][1].any()
    assert dup["labels"].tolist() == [1, 1, 1, 0, 0, 0, 1] and dup["moved"] == 4 and dup["gap"] > 0.01  # the tie itself is no gap
    assert R.assign(R.bf16_to_f64(both), R.bf16_to_f64(both[[0, 6]]))[2] == 0.0
    assert R.run(bits[:1], bits[:1], 3)["gap"] == np.inf  # k = 1: nothing to confuse


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_committed_fixtures_keep_their_margin(name):
    """what test_gpu_kmeans.py asserts again before it compares a whole run: gap > 4 delta, and the generator reproduces them"""
    n, d, kt, k, noise = R.CASES[name]
    x, rows = R.load_case(name)
    g = np.load(os.path.join(R.GOLDEN, f"kmeans_{name}.npz"))
    assert x.shape == (n, d) and x.dtype == np.uint16 and rows.shape == (k,) and len(set(rows.tolist())) == k
    ref = R.run(x, x[rows], 50)
    assert ref["converged"] and ref["iterations"] == int(g["iterations"]) >= 2 and ref["gap"] == float(g["gap"]) > 4 * R.delta(d)
    norms = np.linalg.norm(R.bf16_to_f64(x), axis=1)
    assert np.all(np.abs(norms - 1) < 2.0 ** -7)


def _rows():
    ids = [f"r{i}" for i in range(8)]
    metas = [{"parent_image": f"/p/page{i // 2}.png", "region_type": "advert" if i % 2 else "text", "area_percentage": 1.5 * i} for i in range(8)]
    metas[7] = None
    return ids, metas


def test_cluster_table_medoids_ties_and_an_empty_cluster():
    import json

    ids, metas = _rows()
    labels = [0, 3, 3, 0, 1, 3, 1, 0]
    sim = [0.5, 0.75, 0.9, 0.5, 0.25, 0.9, 0.25, 0.125]
    t = rc.cluster_table(labels, sim, ids, metas, n_clusters=4, iterations=3, converged=True, objective=4.175)
    assert t["n_regions"] == 8 and t["n_clusters"] == 4 and t["n_empty"] == 1 and t["iterations"] == 3 and t["converged"] is True
    assert [c["cluster"] for c in t["clusters"]] == [0, 1, 2, 3] and [c["size"] for c in t["clusters"]] == [3, 2, 0, 3]
    c0, c1, c2, c3 = t["clusters"]
    # members by score descending, the lower row first among equals; the medoid is the first of them
    assert [m["id"] for m in c0["members"]] == ["r0", "r3", "r7"] and c0["medoid"] == "r0"
    assert [m["id"] for m in c3["members"]] == ["r2", "r5", "r1"] and c3["medoid"] == "r2"
    assert [m["id"] for m in c1["members"]] == ["r4", "r6"] and c1["medoid"] == "r4"
    assert c0["cohesion"] == pytest.approx(0.375) and c3["cohesion"] == pytest.approx(0.85) and c1["cohesion"] == 0.25
    assert c2 == {"cluster": 2, "size": 0, "cohesion": None, "medoid": None, "pages": [], "members": []}
    assert c0["pages"] == ["page0.png", "page1.png"] and c3["pages"] == ["page0.png", "page1.png", "page2.png"]
    assert c0["members"][2] == {"id": "r7", "parent_image": "", "type": "unknown", "area_percentage": 0, "score": 0.125}
    assert c3["members"][0] == {"id": "r2", "parent_image": "page1.png", "type": "text", "area_percentage": 3.0, "score": 0.9}
    assert json.loads(json.dumps(t)) == t  # JSON-ready: no numpy scalars
    # n_clusters defaults to the largest label + 1; max_members cuts the lists, not the sizes
    cut = rc.cluster_table(np.array(labels, dtype=np.int32), np.array(sim, dtype=np.float32), ids, metas, max_members=1)
    assert cut["n_clusters"] == 4 and cut["iterations"] is None and [len(c["members"]) for c in cut["clusters"]] == [1, 1, 0, 1]
    assert [c["size"] for c in cut["clusters"]] == [3, 2, 0, 3] and cut["clusters"][0]["cohesion"] == pytest.approx(0.375)
    empty = rc.cluster_table([], [], [], [], n_clusters=0)
    assert empty["clusters"] == [] and empty["n_regions"] == 0
    with pytest.raises(ValueError):
        rc.cluster_table(labels[:-1], sim, ids, metas)
    with pytest.raises(ValueError):
        rc.cluster_table(labels, sim, ids, metas, n_clusters=3)


def _unit_rows(n, d, seed):
    import torch

    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32))
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_start_rows_are_reproducible_distinct_and_sorted(init):
    emb = _unit_rows(200, 64, 0)
    a = rc.kmeans_init_rows(emb, 17, init, seed=5)
    b = rc.kmeans_init_rows(emb, 17, init, seed=5)
    c = rc.kmeans_init_rows(emb, 17, init, seed=6)
    assert a.dtype == np.int32 and a.shape == (17,) and np.array_equal(a, b) and not np.array_equal(a, c)
    for rows in (a, c):
        assert len(set(rows.tolist())) == 17 and rows.min() >= 0 and rows.max() < 200 and np.all(np.diff(rows) > 0)
    every = rc.kmeans_init_rows(emb, 200, init, seed=1)
    assert every.tolist() == list(range(200))
    if init == "random":
        assert np.array_equal(a, np.sort(np.random.default_rng(5).choice(200, size=17, replace=False)))


def test_kmeans_plus_plus_spreads_over_the_blobs_and_survives_copies():
    import torch

    # 4 tight blobs of 50 rows: four k-means++ rows hit four blobs (a uniform draw does so with probability 3/32)
    axes = torch.eye(64)[:4].repeat_interleave(50, dim=0)
    emb = axes + 0.01 * torch.from_numpy(np.random.default_rng(1).standard_normal((200, 64)).astype(np.float32))
    emb = (emb / emb.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    for seed in range(5):
        rows = rc.kmeans_init_rows(emb, 4, "k-means++", seed=seed)
        assert sorted((rows // 50).tolist()) == [0, 1, 2, 3], (seed, rows)
    # a table of copies of two rows: the third row has no distance left to be drawn by, and is still distinct
    two = torch.eye(64)[:2].repeat(5, 1).to(torch.bfloat16)
    rows = rc.kmeans_init_rows(two, 3, "k-means++", seed=0)
    assert len(set(rows.tolist())) == 3 and {int(r) % 2 for r in rows} == {0, 1}


def test_explicit_start_rows_and_refusals():
    emb = _unit_rows(50, 64, 2)
    given = np.array([40, 3, 17], dtype=np.int64)
    assert rc.kmeans_init_rows(emb, 3, given).tolist() == [40, 3, 17] and rc.kmeans_init_rows(emb, 3, [1, 2, 3]).dtype == np.int32
    for bad, msg in [(np.array([1, 1, 2]), "distinct"), (np.array([1, 2, 50]), r"0\.\.49"), (np.array([-1, 2, 5]), r"0\.\.49"),
                     (np.array([1, 2]), "n_clusters = 3"), (np.array([1.0, 2.0, 3.0]), "integer"), (np.array([[1, 2, 3]]), "1-D")]:
        with pytest.raises(ValueError, match=msg):
            rc.kmeans_init_rows(emb, 3, bad)
    with pytest.raises(ValueError, match="'k-means\\+\\+', 'random'"):
        rc.kmeans_init_rows(emb, 3, "farthest")
    for k in (0, 51):
        with pytest.raises(ValueError, match=r"1\.\.50"):
            rc.kmeans_init_rows(emb, k, "random")


class _Rows:
    """a collection of n rows, as far as cluster_regions reads one"""

    def __init__(self, n):
        self.n = n

    def get(self, include=None, where=None):
        self.where = where
        return {"ids": [f"r{i}" for i in range(self.n)], "metadatas": [{"is_region": True}] * self.n, "embeddings": [[1.0] + [0.0] * 63] * self.n}


def test_python_side_refusals_come_before_any_engine():
    """none of these reaches the GPU: engine=None would have to create one"""
    col = _Rows(5)
    for kw, msg in [(dict(n_clusters=0), r"n_clusters = 0 must lie in 1\.\.5"), (dict(n_clusters=6), r"1\.\.5"),
                    (dict(n_clusters=2, n_init=0), "n_init = 0"), (dict(n_clusters=2, max_iter=-1), r"max_iter = -1 must lie in 0\.\.1000"),
                    (dict(n_clusters=2, max_iter=1001), r"0\.\.1000")]:
        with pytest.raises(ValueError, match=msg):
            rc.cluster_regions(col, **kw)
    assert col.where == {"is_region": {"$eq": True}}
    none = rc.cluster_regions(_Rows(0), 3)
    assert none["n_regions"] == 0 and none["clusters"] == []
    sig = inspect.signature(rc.cluster_regions).parameters
    assert sig["init"].default == "k-means++" and sig["seed"].default == 0 and sig["n_init"].default == 1 and sig["max_iter"].default == 100
    assert sig["n_clusters"].default is inspect.Parameter.empty
