"""K19 without a GPU: the float64 reference of tests/hierarchy_reference.py held against K18's and K14's references (the cut
identity), the numpy restatement of the kernels' rounds held against Kruskal's tree (and three mutants of it caught), the host
functions of region_compare on hand-made trees and against scikit-learn's HDBSCAN, the store round trip and the ABI names."""
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
import hierarchy_reference as H  # noqa: E402

from multimodal_embeddings_amd import _lib  # noqa: E402
from multimodal_embeddings_amd import region_compare as rc  # noqa: E402
from multimodal_embeddings_amd import store  # noqa: E402


# ---- (a) the cut identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,seed,min_samples,grouped", H.COMBOS)
def test_the_cut_at_tau_is_k18_s_core_rows_and_clusters(n, d, seed, min_samples, grouped):
    c = H.case(n, d, seed, min_samples, grouped)
    ref = R.case(n, d, seed, min_samples, grouped)["ref"]
    dl = DR.delta(d)
    finite = c["M"][np.isfinite(c["M"])]
    nearest = np.abs(np.concatenate([finite, c["core"]]) - c["tau"]).min()
    print(f"({n}, {d}) min_samples {min_samples} grouped {grouped}: nearest weight to tau at {nearest / dl:.3f} delta")
    assert nearest >= 2 * dl
    labels, kind = H.cut(c["edges"], c["weights"], c["core"], c["tau"])
    is_core = ref["kind"] == 2
    assert np.array_equal(kind == 2, is_core) and is_core.any() and not is_core.all()
    assert np.array_equal(labels[is_core], ref["labels"][is_core]) and (labels[~is_core] == -1).all()
    assert len(c["edges"]) == n - len(set(H.components(c["adm"]).tolist()))
    # the host function gives the same from the same tree
    got_labels, got_kind = rc.cut_hierarchy(c["edges"], c["weights"], c["core"], c["tau"])
    assert np.array_equal(got_labels, labels) and np.array_equal(got_kind, kind) and got_labels.dtype == np.int32


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("n,d,seed", R.CASES[:3])
def test_min_samples_1_is_k14(n, d, seed, grouped):
    c = H.case(n, d, seed, 1, grouped)
    k14 = DR.reference(c["x32"], c["tau"], c["group"])
    assert (c["core"] == H.ABOVE).all()
    labels, kind = rc.cut_hierarchy(c["edges"], c["weights"], c["core"], c["tau"])
    assert np.array_equal(labels, k14["labels"]) and (kind == 2).all()


# ---- (b) the rounds, restated in numpy, give Kruskal's tree ---------------------------------------------------------------------
def _round_inputs():
    x32, _ = H.one_hot(300, 7)
    S = DR.similarity(x32)
    adm = DR.admissible(300)
    for ms in (1, 5):
        yield f"one-hot ms {ms}", H.mutual(S, adm, H.core_similarity(S, adm, ms)), adm
    for n, d, seed in R.CASES[:3]:
        for ms, grouped in ((8, False), (3, True)):
            c = H.case(n, d, seed, ms, grouped)
            yield f"({n}, {d}, {seed}) ms {ms} grouped {grouped}", c["M"], c["adm"]


ROUND_INPUTS = list(_round_inputs())


@pytest.mark.parametrize("name,M,adm", ROUND_INPUTS, ids=[r[0] for r in ROUND_INPUTS])
def test_the_rounds_return_kruskal_s_edge_set(name, M, adm):
    want, _ = H.kruskal(M, adm)
    edges, rounds, cycles = H.boruvka(M, adm)
    print(f"{name}: {len(edges)} edges in {rounds} rounds")
    assert cycles == 0 and len(edges) == len(set(edges))
    assert set(edges) == set(map(tuple, want.tolist()))
    assert rounds <= int(np.ceil(np.log2(len(M)))) + 1


@pytest.mark.parametrize("mutant", ["other_root", "j_descending", "no_mutual_rule"])
def test_a_wrong_tie_rule_is_caught(mutant):
    caught = []
    for name, M, adm in ROUND_INPUTS:
        want, _ = H.kruskal(M, adm)
        edges, _, cycles = H.boruvka(M, adm, mutant)
        if cycles or len(edges) != len(want) or set(edges) != set(map(tuple, want.tolist())):
            caught.append(name)
        if mutant == "no_mutual_rule":  # more edges than a forest has
            assert len(edges) > len(M) - len(set(H.components(adm).tolist())), name
    print(f"{mutant}: caught on {caught}")
    assert caught


# ---- (c) hierarchy_clusters against scikit-learn's HDBSCAN ----------------------------------------------------------------------
def _sklearn_labels(D, min_samples, perm=None):
    from sklearn.cluster import HDBSCAN

    if perm is None:
        return HDBSCAN(metric="precomputed", min_samples=min_samples, min_cluster_size=5).fit(D.copy()).labels_
    out = np.empty(len(D), dtype=np.int64)
    out[perm] = HDBSCAN(metric="precomputed", min_samples=min_samples, min_cluster_size=5).fit(D[np.ix_(perm, perm)].copy()).labels_
    return out


def _moved_rows(mine, theirs):
    """the rows whose cluster in `theirs` is not the one most rows of their cluster in `mine` have"""
    moved = []
    for lab in np.unique(mine):
        rows = np.flatnonzero(mine == lab)
        values, counts = np.unique(theirs[rows], return_counts=True)
        moved.extend(rows[theirs[rows] != values[np.argmax(counts)]].tolist())
    return moved


def test_hierarchy_clusters_agree_with_scikit_learn():
    """scikit-learn's own answer depends on the order of equal weights, so a combination counts only when its partition does not
    move under three row permutations; at least 8 of the 12 must be such (a fixture error otherwise, never a skip)."""
    stable, differ = [], []
    for n, d, seed, ms, grouped in H.COMBOS:
        if grouped:
            continue
        c = H.case(n, d, seed, ms)
        D = np.maximum(0.0, 1.0 - c["S"])
        np.fill_diagonal(D, 0.0)
        base = _sklearn_labels(D, ms)
        if not all(H.same_partition(base, _sklearn_labels(D, ms, np.random.default_rng(s).permutation(n))) for s in (5, 6, 7)):
            continue
        stable.append((n, d, seed, ms))
        got = rc.hierarchy_clusters(c["edges"], c["weights"], c["core"], 5)
        assert (base >= 0).any() and len(set(base[base >= 0].tolist())) >= 2
        if not H.same_partition(got["labels"], base):
            # admitted only when it is traced to an equal-weight merge: every row that moved hangs between two clusters on two
            # tree edges of exactly its own core similarity, which either order of merging may give to either side
            # (DESIGN.md 4.29); without those rows the partitions are equal
            moved = _moved_rows(got["labels"], base)
            e, w = c["edges"], c["weights"]
            tied = all((w[(e == r).any(1)] == c["core"][r]).sum() >= 2 for r in moved)
            keep = np.setdiff1d(np.arange(n), moved)
            assert tied and len(moved) <= 2 and H.same_partition(got["labels"][keep], base[keep]), (n, d, seed, ms, moved)
            differ.append((n, d, seed, ms, moved))
        # the ids are the smallest members; strength is 0 exactly on the noise rows
        lab = got["labels"]
        assert all(lab[r] == np.flatnonzero(lab == lab[r]).min() for r in np.flatnonzero(lab >= 0)[:50])
        assert np.array_equal(got["strength"] > 0, lab >= 0) and got["strength"].max() <= 1.0
        assert set(got["persistence"]) == set(lab[lab >= 0].tolist())
    print(f"stable under the permutations: {len(stable)} of 12: {stable}")
    assert len(stable) >= 8, f"fixture: scikit-learn's partition is stable on {len(stable)} of 12 combinations only"
    print(f"differing only by an equal-weight merge: {differ}")
    assert len(stable) - len(differ) >= 8


# ---- (d) hand-made trees --------------------------------------------------------------------------------------------------------
def _two_blobs_and_a_bridge():
    """rows 0..5 and 7..12 are chains of weight 0.9 .. 0.8, row 6 joins both at 0.3 / 0.25"""
    edges = [(i, i + 1) for i in range(5)] + [(i, i + 1) for i in range(7, 12)] + [(5, 6), (6, 7)]
    weights = [0.9, 0.88, 0.86, 0.84, 0.82] + [0.9, 0.88, 0.86, 0.84, 0.82] + [0.3, 0.25]
    return np.array(edges), np.array(weights), np.full(13, 1.5)


def test_cut_and_linkage_on_two_blobs_and_a_bridge():
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage

    e, w, core = _two_blobs_and_a_bridge()
    labels, kind = rc.cut_hierarchy(e, w, core, 0.5)
    assert labels.tolist() == [0] * 6 + [6] + [7] * 6 and (kind == 2).all()
    assert rc.cut_hierarchy(e, w, core, 0.28)[0].tolist() == [0] * 7 + [7] * 6
    assert rc.cut_hierarchy(e, w, core, 0.2)[0].tolist() == [0] * 13
    assert rc.cut_hierarchy(e, w, core, 0.95)[0].tolist() == list(range(13))
    # a row whose core similarity is below the threshold is noise, whatever its edges weigh
    core2 = core.copy()
    core2[6] = 0.3
    w2 = np.minimum(w, np.where((e == 6).any(1), 0.3, 1.5))
    labels, kind = rc.cut_hierarchy(e, w2, core2, 0.5)
    assert labels[6] == -1 and kind[6] == 0 and (np.delete(kind, 6) == 2).all()
    # the order of the edges does not matter
    perm = np.random.default_rng(0).permutation(len(e))
    assert np.array_equal(rc.cut_hierarchy(e[perm][:, ::-1], w[perm], core, 0.5)[0], rc.cut_hierarchy(e, w, core, 0.5)[0])
    z = rc.linkage_of(e, w)
    assert z.shape == (12, 4) and is_valid_linkage(z) and (np.diff(z[:, 2]) >= 0).all() and z[-1, 3] == 13
    for t in (0.95, 0.85, 0.5, 0.28, 0.2):  # fcluster at the height 1 - t is the cut at t (min_samples = 1)
        flat = fcluster(z, 1.0 - t, criterion="distance")
        assert H.same_partition(flat, rc.cut_hierarchy(e, w, core, t)[0]), t
    with pytest.raises(ValueError, match="forest"):
        rc.linkage_of(e[:-1], w[:-1])
    with pytest.raises(ValueError, match="cycle"):
        rc.linkage_of(np.array([(0, 1), (1, 2), (0, 2)]), np.array([0.5, 0.4, 0.3]))


def test_hierarchy_clusters_on_two_blobs_and_a_bridge():
    e, w, core = _two_blobs_and_a_bridge()
    got = rc.hierarchy_clusters(e, w, core, 5)
    # the root splits at lambda = 1 / 0.75 (the edge of 0.25) into rows 0..6 and rows 7..12; row 6 leaves its cluster first, at
    # 1 / 0.7, then row 5 (12) at 1 / 0.18 (the edge of 0.82), and at 1 / 0.16 the five rows left fall apart into 4 and 1
    assert got["labels"].tolist() == [0] * 7 + [7] * 6
    assert got["strength"][6] == pytest.approx((1 / 0.7) / (1 / 0.16)) and (got["strength"] > 0).all()
    lam = {0.82: 1 / 0.18, 0.84: 1 / 0.16, 0.86: 1 / 0.14, 0.88: 1 / 0.12, 0.9: 1 / 0.1}
    assert set(got["persistence"]) == {0, 7}
    birth = 1 / 0.75
    want = (lam[0.82] - birth) + 5 * (lam[0.84] - birth)
    assert got["persistence"][7] == pytest.approx(want) and got["persistence"][0] == pytest.approx(want + (1 / 0.7 - birth))
    assert got["strength"].max() == 1.0 and got["strength"][5] == pytest.approx(lam[0.82] / lam[0.84])
    # min_cluster_size above a blob: nothing to select but the root, which is not allowed
    none = rc.hierarchy_clusters(e, w, core, 7)
    assert (none["labels"] == -1).all() and none["persistence"] == {}
    one = rc.hierarchy_clusters(e, w, core, 7, allow_single_cluster=True)
    assert set(one["labels"].tolist()) <= {0, -1} and (one["labels"] == 0).sum() >= 7
    with pytest.raises(ValueError, match="min_cluster_size = 1"):
        rc.hierarchy_clusters(e, w, core, 1)


def test_a_chain_all_equal_weights_and_a_forest():
    n = 12
    e = np.array([(i, i + 1) for i in range(n - 1)])
    core = np.full(n, 1.5)
    # a chain of falling weights never splits into two clusters of 3: no cluster, or the root alone
    w = np.linspace(0.9, 0.4, n - 1)
    assert (rc.hierarchy_clusters(e, w, core, 3)["labels"] == -1).all()
    got = rc.hierarchy_clusters(e, w, core, 3, allow_single_cluster=True)
    assert (got["labels"] >= 0).any() and set(got["labels"].tolist()) <= {0, -1}
    # all-equal weights: the merges run in the order of the tree (lo ascending), so the dendrogram is a caterpillar; the cut is
    # all or nothing
    w = np.full(n - 1, 0.5)
    z = rc.linkage_of(e, w)
    assert z[:, 3].tolist() == list(range(2, n + 1)) and (z[:, 2] == 0.5).all()
    assert rc.cut_hierarchy(e, w, core, 0.5)[0].tolist() == [0] * n and rc.cut_hierarchy(e, w, core, 0.51)[0].tolist() == list(range(n))
    assert (rc.hierarchy_clusters(e, w, core, 3)["labels"] == -1).all()
    # weight 1 (identical rows): lambda is infinite, the rows never leave
    two = rc.hierarchy_clusters(np.array([(0, 1), (1, 2), (3, 4), (4, 5), (2, 3)]), np.array([1.0, 1.0, 1.0, 1.0, 0.0]), np.full(6, 1.0), 3)
    assert two["labels"].tolist() == [0, 0, 0, 3, 3, 3] and (two["strength"] == 1.0).all()
    # a forest: the components are joined below every weight; a row without an edge is noise
    f = rc.hierarchy_clusters(np.array([(0, 1), (1, 2), (3, 4), (4, 5)]), np.array([0.9, 0.8, 0.9, 0.8]), np.full(7, 1.5), 3)
    assert f["labels"].tolist() == [0, 0, 0, 3, 3, 3, -1]
    assert rc.cut_hierarchy(np.zeros((0, 2)), np.zeros(0), np.full(3, 1.5), 0.5)[0].tolist() == [0, 1, 2]
    assert rc.hierarchy_clusters(np.zeros((0, 2)), np.zeros(0), np.full(1, 1.5), 2)["labels"].tolist() == [-1]


# ---- (e) region_hierarchy on a stand-in engine, the store, the ABI --------------------------------------------------------------
class _ReferenceEngine:
    """answers Engine.hierarchy from float64 on the CPU, and records what it was given"""

    def __init__(self):
        self.calls = []

    def hierarchy(self, emb, min_samples, group=None):
        self.calls.append({"n": emb.shape[0], "min_samples": min_samples, "group": None if group is None else np.array(group)})
        S = DR.similarity(emb.float().numpy())
        adm = DR.admissible(len(S), group)
        core = H.core_similarity(S, adm, min_samples)
        edges, weights = H.kruskal(H.mutual(S, adm, core), adm)
        return {"edges": edges.astype(np.int32), "weights": weights.astype(np.float32), "core": core.astype(np.float32), "rounds": 3,
                "components": len(S) - len(edges)}


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


def _without_counts(table):
    for c in table["clusters"]:
        for m in c["members"]:
            m.pop("count", None)
    return table


def test_region_hierarchy_on_a_stand_in_engine_and_the_store(monkeypatch, tmp_path):
    monkeypatch.setattr(rc, "to_unit_bf16", _unit_bf16_on_cpu)
    t = R.table(203, 64, 2)
    col, ids, metas = _collection(t["x32"])
    x32 = _unit_bf16_on_cpu(t["x32"], None).float().numpy()
    S = DR.similarity(x32)
    tau, gap = DR.widest_gap(S)
    assert gap >= 4 * DR.delta(64)
    eng = _ReferenceEngine()
    summaries = set()
    for exclude in ("none", "parent", "prefix"):
        h = rc.region_hierarchy(col, 8, exclude=exclude, prefix_length=7, engine=eng)
        call = eng.calls[-1]
        group = rc.duplicate_inputs(metas, exclude, 7)[0]
        assert call["n"] == 203 and call["min_samples"] == 8
        assert (call["group"] is None) if exclude == "none" else np.array_equal(call["group"], group)
        assert h.ids == ids and h.min_samples == 8 and h.rounds == 3 and h.components == 203 - len(h.edges)
        assert h.edges.dtype == np.int32 and h.weights.dtype == np.float32 and h.core.dtype == np.float32
        # .cut(tau) is K18's table with the border rows among the noise
        ref = R.reference(x32, tau, 8, group, S=S)
        is_core = ref["kind"] == 2
        want = rc.density_table(np.where(is_core, ref["labels"], -1), np.where(is_core, 2, 0), ref["count"], np.full(203, -1), np.zeros(203), ids,
                                metas, threshold=tau, min_samples=8)
        got = h.cut(tau)
        assert got == _without_counts(want) and got["summary"]["n_border"] == 0 and got["summary"]["n_core"] == int(is_core.sum())
        summaries.add(json.dumps(got["summary"]))
        cl = h.clusters(5)
        assert cl["n_regions"] == 203 and cl["noise"]["count"] + sum(c["size"] for c in cl["clusters"]) == 203
        assert [c["size"] for c in cl["clusters"]] == sorted((c["size"] for c in cl["clusters"]), reverse=True) and len(cl["clusters"]) >= 2
        assert all(c["size"] >= 5 and len(c["members"]) == c["size"] for c in cl["clusters"])
    assert len(summaries) == 3
    h = rc.region_hierarchy(col, 8, engine=eng)
    assert h.linkage().shape == (202, 4)
    # the store gives every bit back
    path = store.save_hierarchy(h, tmp_path / "trees" / "regions")
    assert path.endswith("regions.npz")
    back = store.load_hierarchy(tmp_path / "trees" / "regions")
    assert back.ids == h.ids and back.min_samples == 8 and back.rounds == h.rounds and back.components == h.components and back.metadatas is None
    for f in ("edges", "weights", "core"):
        assert getattr(back, f).dtype == getattr(h, f).dtype and getattr(back, f).tobytes() == getattr(h, f).tobytes()
    assert back.cut(tau)["summary"] == h.cut(tau)["summary"] and np.array_equal(back.clusters(5)["labels"], h.clusters(5)["labels"])
    # the report
    out = tmp_path / "reports" / "hierarchy.json"
    report = rc.create_hierarchy_report(col, 8, str(out), thresholds=(tau, 0.9), min_cluster_size=5, engine=eng)
    assert json.loads(out.read_text()) == report and len(report["edges"]) == 202 and len(report["cuts"]) == 2
    assert report["cuts"][0]["summary"] == h.cut(tau)["summary"] and set(report["core"]) == set(ids)
    with pytest.raises(ValueError, match="min_samples = 0"):
        rc.region_hierarchy(col, 0, engine=eng)
    with pytest.raises(ValueError, match="exclude"):
        rc.region_hierarchy(col, 8, exclude="page", engine=eng)
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    empty = rc.region_hierarchy(RegionCollection(), 3, engine=eng)
    assert empty.ids == [] and empty.cut(0.5)["n_regions"] == 0 and empty.clusters(5)["clusters"] == []


def test_header_exports_and_engine_name_k19():
    with open(os.path.join(HERE, "..", "include", "mme.h")) as fh:
        header = fh.read()
    for name in ("mme_hierarchy_init", "mme_hierarchy_core", "mme_hierarchy_scan", "mme_hierarchy_merge"):
        assert f"int {name}(mme_ctx* ctx," in header and name in _lib.EXPORTS
    assert "} mme_hierarchy_state;" in header and "#define MME_ABI_VERSION 2" in header
    assert [f for f, _ in _lib._HierarchyState._fields_] == ["core", "comp", "row_key", "parent", "comp_weight", "comp_edge", "edges", "weights",
                                                            "counters"]
    assert [len(_lib.EXPORTS[f"mme_hierarchy_{k}"][1]) for k in ("init", "core", "scan", "merge")] == [4, 10, 9, 4]
    for name in ("hierarchy_init", "hierarchy_core", "hierarchy_scan", "hierarchy_merge", "hierarchy"):
        assert callable(getattr(_lib.Engine, name))
    assert list(inspect.signature(_lib.Engine.hierarchy).parameters) == ["self", "emb", "min_samples", "group"]
    for fn in (rc.region_hierarchy, rc.create_hierarchy_report):
        assert inspect.signature(fn).parameters["min_samples"].default is inspect.Parameter.empty
    assert inspect.signature(rc.region_hierarchy).parameters["exclude"].default == "none"
    build = open(os.path.join(HERE, "..", "multimodal_embeddings_amd", "build.py")).read()
    assert '"hierarchy.hip"' in build and '"capi_hierarchy.hip"' in build and '"hierarchy.h"' in build
