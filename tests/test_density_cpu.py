"""Density clusters (K18) without a GPU: the float64 reference (tests/density_reference.py) against scikit-learn's DBSCAN, the
conditions the GPU cases rely on, the two identities that tie K18 to K14, the report table, the ABI names, and the host
functions of region_compare on a stand-in engine."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import density_reference as R  # noqa: E402
import duplicates_reference as DR  # noqa: E402

from multimodal_embeddings_amd import _lib  # noqa: E402
from multimodal_embeddings_amd import region_compare as rc  # noqa: E402


# ---- (a) the reference is DBSCAN ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("min_samples", [3, 5, 8])
@pytest.mark.parametrize("n,d,seed", R.CASES)
def test_reference_agrees_with_scikit_learn(n, d, seed, min_samples, grouped):
    from sklearn.cluster import DBSCAN

    c = R.case(n, d, seed, min_samples, grouped)
    ref, S, adm = c["ref"], c["S"], c["ref"]["adm"]
    D = np.clip(1.0 - S, 0.0, None)
    D[~adm] = 10.0
    np.fill_diagonal(D, 0.0)
    sk = DBSCAN(eps=1.0 - c["tau"], min_samples=min_samples, metric="precomputed").fit(D)
    core = np.zeros(n, dtype=bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(core, ref["kind"] == 2)
    # the partition of the core rows, up to renaming
    pairs = set(zip(sk.labels_[core].tolist(), ref["labels"][core].tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) == ref["summary"][1]
    assert np.array_equal(sk.labels_ == -1, ref["kind"] == 0)
    # scikit-learn gives a border row to the cluster that reaches it first: one of its core neighbours' clusters, not always
    # the most similar one's
    to_ref = dict(pairs)
    E = adm & (S >= c["tau"])
    differ = 0
    for r in np.flatnonzero(ref["kind"] == 1):
        near = np.flatnonzero(E[r] & core)
        assert to_ref[int(sk.labels_[r])] in set(ref["labels"][near].tolist())
        differ += to_ref[int(sk.labels_[r])] != ref["labels"][r]
    print(f"border rows scikit-learn places elsewhere: {differ}")
    assert ref["summary"][2] > 0 and ref["summary"][3] > 0  # core and border rows at every min_samples


# ---- (b) the conditions the GPU cases rely on --------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("n,d,seed", R.CASES)
def test_cases_have_one_right_answer(n, d, seed, grouped):
    for min_samples in (3, 8):
        c = R.case(n, d, seed, min_samples, grouped)
        assert DR.WINDOW[0] < c["tau"] < DR.WINDOW[1]
        R.check_fixture(c)
        assert (c["ref"]["summary"][2:4] > 0).all() and (min_samples == 3 or c["ref"]["summary"][4] > 0), c["ref"]["summary"]


def test_the_bridged_case_tells_dbscan_from_single_linkage():
    c = R.case(203, 64, 2, 8)
    k14 = DR.reference(c["x32"], c["tau"])
    assert c["ref"]["summary"][1] == 12 and k14["summary"][1] == 10
    assert c["ref"]["two_clusters"].sum() == 4


def test_the_issue_s_figures():
    want = {(203, 64, 1): (172, 28, 3, 10), (203, 64, 2): (174, 26, 3, 12), (331, 128, 1): (275, 51, 5, 17), (515, 256, 1): (401, 109, 5, 27),
            (515, 768, 1): (450, 62, 3, 25), (643, 1024, 1): (538, 100, 5, 31)}
    for key, (core, border, noise, clusters) in want.items():
        s = R.case(*key, 8)["ref"]["summary"].tolist()
        assert s[1:5] == [clusters, core, border, noise], (key, s)


# ---- (c) the two identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("n,d,seed", R.CASES[1:4])
def test_min_samples_1_and_2_are_k14(n, d, seed, grouped):
    t = R.table(n, d, seed)
    group = R.group_ids(n, seed) if grouped else None
    k14 = DR.reference(t["x32"], t["tau"], group)
    one = R.reference(t["x32"], t["tau"], 1, group, S=t["S"])
    assert (one["kind"] == 2).all() and np.array_equal(one["labels"], k14["labels"]) and np.array_equal(one["count"], k14["degree"])
    assert one["summary"].tolist() == [len(k14["edges"]), len(set(k14["labels"].tolist())), n, 0, 0, np.bincount(k14["labels"]).max()]
    two = R.reference(t["x32"], t["tau"], 2, group, S=t["S"])
    single = np.bincount(k14["labels"], minlength=n)[k14["labels"]] == 1
    assert not (two["kind"] == 1).any() and np.array_equal(two["kind"] == 0, single)
    assert np.array_equal(two["labels"], np.where(single, -1, k14["labels"]))
    assert two["summary"].tolist() == [k14["summary"][0], k14["summary"][1], k14["summary"][2], 0, int(single.sum()), k14["summary"][3]]


def test_reference_on_a_star():
    x32 = star()[0]
    S = DR.similarity(x32)
    off = S[np.triu_indices(13, 1)]
    assert abs(S[0, 1:] - 0.8).max() < 0.01 and abs(off[12:] - 0.64).max() < 0.01
    ref = R.reference(x32, 0.7, 13)
    assert ref["kind"].tolist() == [2] + [1] * 12 and (ref["labels"] == 0).all() and ref["border_idx"].tolist() == [-1] + [0] * 12
    assert ref["summary"].tolist() == [12, 1, 1, 12, 0, 13]
    assert R.reference(x32, 0.7, 14)["summary"].tolist() == [12, 0, 0, 0, 13, 0]


def star(d=64):
    """a centre row and 12 rows at cosine 0.8 to it and 0.64 to each other: (rows as bf16-valued float32, bf16 tensor)"""
    x = np.zeros((13, d))
    x[:, 0] = 1.0
    x[np.arange(1, 13), np.arange(1, 13)] = 0.75
    return DR.to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


# ---- (d) the report table -----------------------------------------------------------------------------------------------------
def _rows(n=10):
    ids = [f"r{i}" for i in range(n)]
    metas = [{"parent_image": f"/p/page{i // 2}.png", "region_type": "text", "box_str": f"{i},0,{i + 5},9"} for i in range(n)]
    metas[9] = None
    return ids, metas


def test_density_table_orders_renumbers_and_lists_noise():
    ids, metas = _rows()
    #          r0  r1  r2  r3  r4  r5  r6  r7  r8  r9
    labels = [3, 1, 1, -1, 3, 1, 7, 3, -1, 7]
    kind = [1, 2, 2, 0, 2, 1, 2, 2, 0, 2]
    count = [1, 2, 2, 0, 2, 1, 1, 2, 0, 1]
    bidx = [4, -1, -1, -1, -1, 2, -1, -1, -1, -1]
    bsim = [0.7, 0, 0, 0, 0, 0.75, 0, 0, 0, 0]
    t = rc.density_table(labels, kind, count, bidx, bsim, ids, metas, threshold=0.65, min_samples=3)
    assert t["threshold"] == 0.65 and t["min_samples"] == 3 and t["n_regions"] == 10
    # size descending, then the first member: {r0, r4, r7} before {r1, r2, r5}, then {r6, r9}; renumbered in that order
    assert [(c["cluster"], c["size"], c["members"][0]["id"]) for c in t["clusters"]] == [(0, 3, "r0"), (1, 3, "r1"), (2, 2, "r6")]
    first = t["clusters"][0]
    assert (first["n_core"], first["n_border"]) == (2, 1) and first["pages"] == ["page0.png", "page2.png", "page3.png"]
    assert first["members"][0] == {"id": "r0", "parent_image": "page0.png", "box": [0.0, 0.0, 5.0, 9.0], "kind": "border", "count": 1,
                                   "best_core": {"id": "r4", "score": 0.7}}
    assert first["members"][1] == {"id": "r4", "parent_image": "page2.png", "box": [4.0, 0.0, 9.0, 9.0], "kind": "core", "count": 2}
    assert t["clusters"][1]["members"][2]["best_core"] == {"id": "r2", "score": 0.75}
    assert t["clusters"][2]["members"][1] == {"id": "r9", "parent_image": "", "box": None, "kind": "core", "count": 1}  # no metadata
    assert t["noise"] == {"count": 2, "ids": ["r3", "r8"]}
    assert t["summary"] == {"n_clusters": 3, "n_core": 6, "n_border": 2, "n_noise": 2, "largest_cluster": 3}
    assert json.loads(json.dumps(t)) == t  # JSON-ready: no numpy scalars
    # min_size drops the tail and keeps the numbers; max_members cuts the lists, not the counts
    big = rc.density_table(labels, kind, count, bidx, bsim, ids, metas, threshold=0.65, min_samples=3, min_size=3)
    assert [c["cluster"] for c in big["clusters"]] == [0, 1] and big["summary"] == t["summary"]
    cut = rc.density_table(labels, kind, count, bidx, bsim, ids, metas, threshold=0.65, min_samples=3, max_members=1)
    assert [len(c["members"]) for c in cut["clusters"]] == [1, 1, 1] and [c["size"] for c in cut["clusters"]] == [3, 3, 2]
    assert cut["clusters"][0]["n_border"] == 1
    empty = rc.density_table([], [], [], [], [], [], [], threshold=None, min_samples=2)
    assert empty["clusters"] == [] and empty["noise"] == {"count": 0, "ids": []} and empty["summary"]["largest_cluster"] == 0
    with pytest.raises(ValueError, match="one entry per row"):
        rc.density_table(labels[:-1], kind, count, bidx, bsim, ids, metas, threshold=0.65, min_samples=3)
    with pytest.raises(ValueError, match="noise rows"):
        rc.density_table([0] * 10, kind, count, bidx, bsim, ids, metas, threshold=0.65, min_samples=3)


# ---- (e) the ABI ----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_engine_name_k18():
    with open(os.path.join(HERE, "..", "include", "mme.h")) as fh:
        header = fh.read()
    for name in ("mme_density_init", "mme_density_count", "mme_density_link", "mme_density_finish"):
        assert f"int {name}(mme_ctx* ctx," in header and name in _lib.EXPORTS
    assert "} mme_density_state;" in header and "#define MME_ABI_VERSION 2" in header
    assert [f for f, _ in _lib._DensityState._fields_] == ["count", "parent", "border", "counters"]
    assert len(_lib.EXPORTS["mme_density_count"][1]) == 10 and len(_lib.EXPORTS["mme_density_link"][1]) == 11
    assert len(_lib.EXPORTS["mme_density_init"][1]) == 4 and len(_lib.EXPORTS["mme_density_finish"][1]) == 10
    for name in ("density_init", "density_count", "density_link", "density_finish", "density_clusters"):
        assert callable(getattr(_lib.Engine, name))
    assert list(inspect.signature(_lib.Engine.density_clusters).parameters) == ["self", "emb", "min_sim", "min_samples", "group"]
    build = open(os.path.join(HERE, "..", "multimodal_embeddings_amd", "build.py")).read()
    assert '"density.hip"' in build and '"capi_density.hip"' in build and '"union_find.h"' in build and '"density.h"' in build


def test_threshold_and_min_samples_have_no_defaults():
    for fn in (rc.density_clusters, rc.create_density_report):
        p = inspect.signature(fn).parameters
        assert p["threshold"].default is inspect.Parameter.empty and p["min_samples"].default is inspect.Parameter.empty
    p = inspect.signature(rc.density_clusters).parameters
    assert p["exclude"].default == "none" and p["min_size"].default == 1 and p["where"].default == {"is_region": {"$eq": True}}
    assert inspect.signature(rc.kth_neighbour_similarity).parameters["exclude"].default == "none"


# ---- (f) the host functions on a stand-in engine ----------------------------------------------------------------------------
class _ReferenceEngine:
    """answers Engine.density_clusters and Engine.neighbours from float64 on the CPU, and records what it was given"""

    def __init__(self):
        self.calls = []

    def density_clusters(self, emb, min_sim, min_samples, group=None):
        self.calls.append({"n": emb.shape[0], "min_sim": min_sim, "min_samples": min_samples, "group": None if group is None else np.array(group)})
        ref = R.reference(emb.float().numpy(), min_sim, min_samples, group)
        return {k: ref[k] for k in ("labels", "kind", "count", "border_idx", "border_sim", "summary")}

    def neighbours(self, emb, group=None, *, fetch, top_n):
        self.calls.append({"fetch": fetch, "top_n": top_n, "group": None if group is None else np.array(group)})
        S = DR.similarity(emb.float().numpy())
        n = len(S)
        idx, sim = np.full((n, top_n), -1, dtype=np.int32), np.zeros((n, top_n), dtype=np.float32)
        for r in range(n):
            order = np.argsort(-S[r], kind="stable")[:fetch]
            keep = [j for j in order if j != r and (group is None or group[j] != group[r])][:top_n]
            idx[r, : len(keep)], sim[r, : len(keep)] = keep, S[r, keep]
        return idx, sim


def _unit_bf16_on_cpu(vecs, engine):
    x = torch.tensor(np.asarray(vecs, dtype=np.float32))
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def _collection(x32, pages=6):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    n = len(x32)
    page = np.random.default_rng(11).integers(0, pages, n)
    metas = [{"parent_image": f"/scans/issue{page[r] // 2:02d}_page{page[r]:02d}.png", "region_type": "text", "box_str": f"{r},{r},{r + 9},{r + 9}",
              "is_region": True} for r in range(n)]
    ids = [f"region_{r:04d}" for r in range(n)]
    col = RegionCollection()
    col.upsert(ids=ids + ["hole_a", "hole_b", "page_0"], embeddings=[v.tolist() for v in x32] + [x32[0].tolist(), x32[1].tolist(), x32[0].tolist()],
               metadatas=metas + [dict(metas[0]), dict(metas[1]), {"is_region": False}])
    col.update(ids=["hole_a", "hole_b"], embeddings=[None, []])  # two regions without an embedding: left out
    return col, ids, metas


def test_density_clusters_and_the_knee_curve_on_a_stand_in_engine(monkeypatch, tmp_path):
    monkeypatch.setattr(rc, "to_unit_bf16", _unit_bf16_on_cpu)
    t = R.table(203, 64, 2)
    col, ids, metas = _collection(t["x32"])
    x32 = _unit_bf16_on_cpu(t["x32"], None).float().numpy()
    eng = _ReferenceEngine()
    tables = {}
    for exclude in ("none", "parent", "prefix"):
        got = rc.density_clusters(col, t["tau"], 8, exclude=exclude, prefix_length=7, engine=eng)
        call = eng.calls[-1]
        group = rc.duplicate_inputs(metas, exclude, 7)[0]
        assert call["n"] == 203 and call["min_samples"] == 8 and call["min_sim"] == t["tau"]
        assert (call["group"] is None) if exclude == "none" else np.array_equal(call["group"], group)
        ref = R.reference(x32, t["tau"], 8, group)
        want = rc.density_table(ref["labels"], ref["kind"], ref["count"], ref["border_idx"], ref["border_sim"], ids, metas, threshold=t["tau"],
                                min_samples=8)
        assert got == want and got["n_regions"] == 203
        tables[exclude] = got
    assert len({json.dumps(v["summary"]) for v in tables.values()}) == 3  # the three rules give three answers
    assert len(set(rc.duplicate_inputs(metas, "prefix", 7)[0].tolist())) == 3 and len(set(rc.duplicate_inputs(metas, "parent", 7)[0].tolist())) == 6
    out = tmp_path / "reports" / "density.json"
    report = rc.create_density_report(col, t["tau"], 8, str(out), min_size=10, engine=eng)
    assert json.loads(out.read_text()) == report and all(c["size"] >= 10 for c in report["clusters"])
    with pytest.raises(ValueError, match="min_samples = 0"):
        rc.density_clusters(col, t["tau"], 0, engine=eng)
    with pytest.raises(ValueError, match="exclude"):
        rc.density_clusters(col, t["tau"], 8, exclude="page", engine=eng)

    # the knee curve: the k-th best admissible similarity of every row, descending
    S = DR.similarity(x32)
    for exclude, k in (("none", 1), ("none", 7), ("parent", 7)):
        got = rc.kth_neighbour_similarity(col, k, exclude=exclude, engine=eng)
        group = rc.duplicate_inputs(metas, exclude)[0]
        Sa = np.where(DR.admissible(203, group), S, -np.inf)
        want = np.sort(-np.sort(-Sa, axis=1)[:, k - 1])[::-1]
        assert got.dtype == np.float32 and got.shape == (203,) and np.array_equal(got, want.astype(np.float32))
        assert eng.calls[-1]["top_n"] == k and eng.calls[-1]["fetch"] == (k + 1 if exclude == "none" else 128)
    for k, exclude in ((0, "none"), (128, "none"), (129, "parent")):
        with pytest.raises(ValueError, match="fetch <= 128"):
            rc.kth_neighbour_similarity(col, k, exclude=exclude, engine=eng)
    # a list that K12's limit cut short is an error by name, a row that has no k-th admissible row at all is left out
    one_page = [dict(m, parent_image="/scans/issue00_page00.png") if r < 150 else m for r, m in enumerate(metas)]
    col.update(ids=ids, metadatas=one_page)
    with pytest.raises(ValueError, match="fetch = 128"):
        rc.kth_neighbour_similarity(col, 40, exclude="parent", engine=eng)
    col.update(ids=ids, metadatas=[dict(m, parent_image="/scans/issue00_page00.png") for m in metas])
    assert rc.kth_neighbour_similarity(col, 1, exclude="parent", engine=eng).shape == (0,)
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    assert rc.density_clusters(RegionCollection(), 0.6, 3, engine=eng)["n_regions"] == 0
    assert rc.kth_neighbour_similarity(RegionCollection(), 3, engine=eng).shape == (0,)
