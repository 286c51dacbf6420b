"""K19 cluster hierarchy (mme_hierarchy_*, Engine.hierarchy*, region_compare.region_hierarchy) against the float64 reference of
tests/hierarchy_reference.py and against K18 / K14 on the same tables.

The tree is defined over the f32 cosines the GEMM writes, so against float64 the edge SET has one right answer only where no
two weights lie within delta of each other; what always has one is asserted instead: the forest properties, every weight within
delta of the float64 weight of its endpoints, the sorted weights within delta of Kruskal's (the k-th largest tree weight is a
max-min quantity, 1-Lipschitz in the sup norm of the weights), and every cut at a threshold 2 delta away from every weight.
On exact inputs (one-hot rows, identical rows, the star) the edge set itself is compared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as R  # noqa: E402
import duplicates_reference as DR  # noqa: E402
import hierarchy_reference as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    return Engine(0)


def _host(res):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


_runs = {}


def _case_run(engine, n, d, seed, min_samples, grouped):
    """the GPU tree of one combination, computed once and shared (read-only)"""
    key = (n, d, seed, min_samples, grouped)
    if key not in _runs:
        c = H.case(n, d, seed, min_samples, grouped)
        _runs[key] = _host(engine.hierarchy(c["xb"].cuda(), min_samples, c["group"]))
    return _runs[key]


def _edge_set(edges):
    return set(map(tuple, np.asarray(edges).reshape(-1, 2).tolist()))


def _in_tree_order(got):
    e, w = got["edges"].astype(np.int64), got["weights"]
    key = list(zip((-w.astype(np.float64)).tolist(), e[:, 0].tolist(), e[:, 1].tolist()))
    return key == sorted(key)


def _check_forest(got, adm):
    """what holds for every input: a spanning forest of the admissible graph, (lo, hi) with lo < hi, in the tree's order"""
    n = len(adm)
    e = got["edges"]
    want_comp = H.components(adm)
    assert e.dtype == np.int32 and e.shape == (n - got["components"], 2) and got["weights"].shape == (len(e),) and got["core"].shape == (n,)
    assert got["components"] == len(set(want_comp.tolist()))
    assert (e[:, 0] < e[:, 1]).all() and (e >= 0).all() and (e < n).all() and adm[e[:, 0], e[:, 1]].all()
    assert len(_edge_set(e)) == len(e)
    top = list(range(n))
    for a, b in e.tolist():  # a host union-find meets no cycle
        while top[a] != a:
            a = top[a]
        while top[b] != b:
            b = top[b]
        assert a != b
        top[max(a, b)] = min(a, b)
    assert np.array_equal(H.components(e, n), want_comp)
    assert _in_tree_order(got)
    assert 0 <= got["rounds"] <= int(np.ceil(np.log2(max(n, 2)))) + 1


# ---- 0. the premise of full-row scans -------------------------------------------------------------------------------------------
def test_the_cosine_block_is_bitwise_symmetric(engine):
    xb = R.table(515, 768, 1)["xb"].cuda()
    ld = 516
    out = torch.full((515, ld), 7.0, dtype=torch.float32, device="cuda")
    engine.gemm_apply(4, xb, xb, outf=out, ldf=ld)
    torch.cuda.synchronize()
    s = out[:, :515].cpu().numpy()
    assert np.isfinite(s).all() and np.abs(s - R.table(515, 768, 1)["S"]).max() <= DR.delta(768)
    assert s.view(np.uint32).tobytes() == np.ascontiguousarray(s.T).view(np.uint32).tobytes()


# ---- 1. - 4. the main cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,seed,min_samples,grouped", H.COMBOS)
def test_forest_weights_and_the_cut_at_tau(engine, n, d, seed, min_samples, grouped):
    c = H.case(n, d, seed, min_samples, grouped)
    k18 = R.case(n, d, seed, min_samples, grouped)
    R.check_fixture(k18)
    dl = DR.delta(d)
    assert np.abs(np.concatenate([c["M"][np.isfinite(c["M"])], c["core"]]) - c["tau"]).min() >= 2 * dl
    got = _case_run(engine, n, d, seed, min_samples, grouped)
    _check_forest(got, c["adm"])
    assert got["components"] == 1
    # 2. core within delta
    err_core = np.abs(got["core"].astype(np.float64) - c["core"]).max()
    # 3. every weight within delta of the float64 weight of its endpoints, the sorted weights within delta of Kruskal's
    e = got["edges"]
    err_edge = np.abs(got["weights"].astype(np.float64) - c["M"][e[:, 0], e[:, 1]]).max()
    err_sorted = np.abs(got["weights"].astype(np.float64) - c["weights"]).max()  # both sorted descending
    print(f"({n}, {d}) ms {min_samples} grouped {grouped}: {got['rounds']} rounds; core {err_core / dl:.3f}, edge {err_edge / dl:.3f}, "
          f"sorted {err_sorted / dl:.3f} delta; {len(_edge_set(e) ^ _edge_set(c['edges']))} edges differ from the float64 tree")
    assert err_core <= dl and err_edge <= dl and err_sorted <= dl
    # 4. the cut at tau: K18's core rows and K18's labels on them, from the GPU and from float64
    from multimodal_embeddings_amd import region_compare as rc

    labels, kind = rc.cut_hierarchy(e, got["weights"], got["core"], c["tau"])
    dens = _host(engine.density_clusters(c["xb"].cuda(), c["tau"], min_samples, c["group"]))
    is_core = dens["kind"] == 2
    assert np.array_equal(kind == 2, is_core) and np.array_equal(labels[is_core], dens["labels"][is_core]) and (labels[~is_core] == -1).all()
    ref = k18["ref"]
    assert np.array_equal(is_core, ref["kind"] == 2) and np.array_equal(labels[is_core], ref["labels"][is_core])
    want_labels, want_kind = H.cut(c["edges"], c["weights"], c["core"], c["tau"])
    assert np.array_equal(labels, want_labels) and np.array_equal(kind, want_kind)


@pytest.mark.parametrize("grouped", [False, True])
def test_min_samples_1_is_k14(engine, grouped):
    from multimodal_embeddings_amd import region_compare as rc

    c = H.case(331, 128, 1, 1, grouped)
    xb = c["xb"].cuda()
    got = _host(engine.hierarchy(xb, 1, c["group"]))
    _check_forest(got, c["adm"])
    assert (got["core"] == 1.5).all()
    k14 = _host(engine.duplicates(xb, c["group"], min_sim=c["tau"]))
    labels, kind = rc.cut_hierarchy(got["edges"], got["weights"], got["core"], c["tau"])
    assert np.array_equal(labels, k14["labels"]) and (kind == 2).all() and len(set(labels.tolist())) > 5
    assert np.array_equal(labels, DR.reference(c["x32"], c["tau"], c["group"])["labels"])


def test_core_similarities_at_the_ends_of_min_samples(engine):
    c = H.case(203, 64, 1, 3, True)
    xb, S, adm, dl = c["xb"].cuda(), c["S"], c["adm"], DR.delta(64)
    partners = adm.sum(1)
    for ms in (1, 2, int(partners.min()) + 1, int(partners.min()) + 2, int(partners.max()) + 1, int(partners.max()) + 2, 204, 2 ** 31 - 1):
        want = H.core_similarity(S, adm, ms)
        st = engine.hierarchy_init(203)
        engine.hierarchy_core(st, xb, c["group"], min_samples=ms)
        got = _host({"core": st["core"][:203]})["core"].astype(np.float64)
        exact = (want == H.BELOW) | (want == H.ABOVE)
        assert np.array_equal(got[exact], want[exact]) and np.abs(got - want).max() <= dl, ms
        if ms == int(partners.min()) + 2:  # beyond some rows' admissible partners under groups, not beyond others'
            assert (want == H.BELOW).any() and not (want == H.BELOW).all()
    assert (want == H.BELOW).all()
    # min_samples = N on 40 identical rows: the last of the 39 partners; N + 1: none
    v = np.random.default_rng(3).standard_normal(64)
    x32, xb = DR.to_bf16(np.tile(v / np.linalg.norm(v), (40, 1)))
    s = float(DR.similarity(x32)[0, 1])
    for ms, want in ((40, s), (41, H.BELOW), (2, s)):
        got = _host(engine.hierarchy(xb.cuda(), ms))
        assert np.abs(got["core"].astype(np.float64) - want).max() <= (0 if want == H.BELOW else dl)
        assert len(set(got["core"].tolist())) == 1 and _edge_set(got["edges"]) == {(0, j) for j in range(1, 40)}


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------
def test_one_hot_rows_across_the_workspace_chunks(engine):
    """N = 40 000 rows of 61 classes x_i = e_(i mod 61) (K18's input: 6.4 GB of cosine values per pass, several chunks): every
    weight is exactly 1 or 0, so the tree is Kruskal's under the strict order, known without an N^2 reference -- a star on the
    first row of every class, and the first rows joined to row 0."""
    from multimodal_embeddings_amd import region_compare as rc

    n, d, k = 40000, 64, 61
    cls = torch.arange(n, device="cuda") % k
    xb = torch.zeros((n, d), dtype=torch.bfloat16, device="cuda")
    xb[torch.arange(n, device="cuda"), cls] = 1.0
    got = _host(engine.hierarchy(xb, 5))
    e, w = got["edges"], got["weights"]
    assert e.shape == (n - 1, 2) and got["components"] == 1 and (got["core"] == 1.0).all() and got["rounds"] <= 3
    assert (w[: n - k] == 1.0).all() and (w[n - k:] == 0.0).all() and _in_tree_order(got)
    want = {(i % k, i) for i in range(k, n)} | {(0, j) for j in range(1, k)}
    assert _edge_set(e) == want
    c = np.arange(n) % k
    for t in (1e-6, 0.5, 1.0):  # every cut in (0, 1] gives the 61 classes
        labels, kind = rc.cut_hierarchy(e, w, got["core"], t)
        assert np.array_equal(labels, c) and (kind == 2).all()
    assert (rc.cut_hierarchy(e, w, got["core"], 0.0)[0] == 0).all()
    # 8. HDBSCAN's clusters of the same tree: the 61 classes, no noise
    h = rc.RegionHierarchy(e, w, got["core"], 5, [f"r{i}" for i in range(n)])
    cl = h.clusters(5)
    assert np.array_equal(cl["labels"], c) and cl["noise"]["count"] == 0 and len(cl["clusters"]) == k
    assert [x["size"] for x in cl["clusters"]] == [656] * 45 + [655] * 16


def test_identical_rows_are_one_star_on_row_0(engine):
    n, d = 500, 64
    v = np.random.default_rng(3).standard_normal(d)
    xb = DR.to_bf16(np.tile(v / np.linalg.norm(v), (n, 1)))[1].cuda()
    for ms in (1, 5, 500):
        got = _host(engine.hierarchy(xb, ms))
        assert _edge_set(got["edges"]) == {(0, j) for j in range(1, n)} and got["components"] == 1 and len(set(got["weights"].tolist())) == 1
        assert got["edges"][:, 1].tolist() == list(range(1, n))  # sorted: equal weights, lo = 0, hi ascending
    got = _host(engine.hierarchy(xb, 501))
    assert (got["core"] == -2.0).all() and (got["weights"] == -2.0).all() and _edge_set(got["edges"]) == {(0, j) for j in range(1, n)}


def _star(d=64):
    """K18's star: a centre row c and 12 rows normalise(c + 0.75 e_k): cosine 0.8 to the centre, 0.64 to each other"""
    x = np.zeros((13, d))
    x[:, 0] = 1.0
    x[np.arange(1, 13), np.arange(1, 13)] = 0.75
    return DR.to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


@pytest.mark.parametrize("permuted", [False, True])
def test_a_star_in_order_and_permuted(engine, permuted):
    """two products per cosine: the f32 values tie exactly where the float64 values do, so the edge set is Kruskal's"""
    x32, xb = _star()
    if permuted:
        perm = np.random.default_rng(4).permutation(13)
        x32, xb = x32[perm], xb[torch.from_numpy(perm)]
    S, adm = DR.similarity(x32), DR.admissible(13)
    centre = int(np.flatnonzero(x32[:, 1:].max(1) == 0)[0])
    for ms in (1, 2, 3, 13, 14):
        core = H.core_similarity(S, adm, ms)
        want, want_w = H.kruskal(H.mutual(S, adm, core), adm)
        got = _host(engine.hierarchy(xb.cuda(), ms))
        _check_forest(got, adm)
        assert _edge_set(got["edges"]) == _edge_set(want), ms
        assert np.abs(got["weights"].astype(np.float64) - want_w).max() <= DR.delta(64)
        if ms <= 2:  # every row's best partner is the centre
            assert _edge_set(got["edges"]) == {(min(centre, j), max(centre, j)) for j in range(13) if j != centre}


# ---- 6. row shards ---------------------------------------------------------------------------------------------------------------
def _pieces(engine, xb, group, min_samples, core_ranges, scan_ranges):
    n = xb.shape[0]
    st = engine.hierarchy_init(n)
    for row0, nrows in core_ranges:
        engine.hierarchy_core(st, xb, group, min_samples=min_samples, row0=row0, nrows=nrows)

    def scan():
        for row0, nrows in scan_ranges:
            engine.hierarchy_scan(st, xb, group, row0=row0, nrows=nrows)

    n_edges, rounds = engine.hierarchy_rounds(st, scan)
    edges, weights = engine.hierarchy_sorted(st, n_edges)
    return _host({"edges": edges, "weights": weights, "core": st["core"][:n], "counters": st["counters"], "rounds": rounds, "components": n - n_edges})


def test_row_shards_and_two_runs_are_bit_equal(engine):
    """core over ranges that start at rows 37, 38 (no multiple of 4) and 300 (past the first 256-row tile), in any order; every
    round's scan over two ranges: a pair's f32 value must not depend on the chunk its row falls in."""
    c = H.case(515, 256, 1, 8, True)
    xb = c["xb"].cuda()
    whole = _host(engine.hierarchy(xb, 8, c["group"]))
    again = _host(engine.hierarchy(xb, 8, c["group"]))
    parts = _pieces(engine, xb, c["group"], 8, [(300, 215), (37, 1), (100, 0), (0, 37), (515, 0), (38, 262)], [(0, 200), (200, 315)])
    other = _pieces(engine, xb, c["group"], 8, [(0, 515)], [(200, 315), (515, 0), (0, 200)])
    for b in (again, parts, other):
        for k in ("edges", "weights", "core"):
            assert whole[k].tobytes() == b[k].tobytes() and whole[k].shape == b[k].shape, k
        assert (b["rounds"], b["components"]) == (whole["rounds"], whole["components"])
    # the counters agree with the arrays: edges emitted, rounds run, components left
    assert parts["counters"].tolist() == [514, whole["rounds"], 1] and whole["rounds"] >= 2


# ---- 7. small N, forests and refusals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
def test_tiny_tables(engine, n):
    x32, xb = R.blobs(n, 64, 7)
    S, adm = DR.similarity(x32), DR.admissible(n)
    for ms in (1, 2, n, n + 1):
        core = H.core_similarity(S, adm, ms)
        want, want_w = H.kruskal(H.mutual(S, adm, core), adm)
        got = _host(engine.hierarchy(xb.cuda(), ms))
        _check_forest(got, adm)
        assert got["components"] == 1 and len(got["edges"]) == n - 1
        assert np.abs(got["core"].astype(np.float64) - core).max() <= DR.delta(64)
        if n > 1:
            assert np.abs(got["weights"].astype(np.float64) - want_w).max() <= DR.delta(64)
            if ms <= n:  # gaps far above delta between five random rows; beyond n every weight is -2.0
                assert _edge_set(got["edges"]) == _edge_set(want)


def test_one_group_has_no_edge_and_a_single_row_group_is_the_hub(engine):
    """Groups are cliques of pairs that never count, so the admissible graph is complete multipartite: without an edge when one
    group holds every row (N components), connected otherwise.  With one row in a group of its own and all others in
    another, that row is every row's only partner: the tree is the star on it, whatever the similarities are."""
    c = H.case(203, 64, 1, 3)
    xb = c["xb"].cuda()
    got = _host(engine.hierarchy(xb, 3, np.zeros(203, dtype=np.int32)))
    _check_forest(got, DR.admissible(203, np.zeros(203)))
    assert got["components"] == 203 and got["edges"].shape == (0, 2) and (got["core"] == -2.0).all() and got["rounds"] <= 1
    group = np.zeros(203, dtype=np.int32)
    group[77] = 1
    adm = DR.admissible(203, group)
    for ms in (1, 2, 3):
        got = _host(engine.hierarchy(xb, ms, group))
        _check_forest(got, adm)
        assert _edge_set(got["edges"]) == {(min(77, j), max(77, j)) for j in range(203) if j != 77}
        core = H.core_similarity(c["S"], adm, ms)
        M = H.mutual(c["S"], adm, core)
        assert np.abs(got["weights"].astype(np.float64) - M[got["edges"][:, 0], got["edges"][:, 1]]).max() <= DR.delta(64)
        assert ((got["core"] == -2.0).sum() == 202) if ms == 3 else (got["core"] > -1.5).all()


def test_refusals_name_the_field_and_leave_the_state_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError

    c = H.case(331, 128, 1, 8, True)
    n = 331
    xb, g = c["xb"].cuda(), torch.from_numpy(c["group"]).cuda()
    before = _host(engine.hierarchy(xb, 8, g))
    st = engine.hierarchy_init(n)
    core = lambda state, emb=xb, **kw: engine.hierarchy_core(state, emb, g, **{"min_samples": 8, **kw})  # noqa: E731
    scan = lambda state, emb=xb, **kw: engine.hierarchy_scan(state, emb, g, **kw)  # noqa: E731

    def refused(match, fn, *a, **kw):
        with pytest.raises(MmeError, match=match):
            fn(*a, **kw)

    fields = ("core", "comp", "row_key", "parent", "comp_weight", "comp_edge", "edges", "weights", "counters")
    for who, fn in (("mme_hierarchy_core", core), ("mme_hierarchy_scan", scan)):
        refused(rf"{who}: d = 96", fn, st, emb=torch.zeros((n, 96), dtype=torch.bfloat16, device="cuda"))
        refused(rf"{who}: rows \[row0 = 300, row0 \+ nrows = 332\)", fn, st, row0=300, nrows=32)
        refused(rf"{who}: rows \[row0 = -1", fn, st, row0=-1, nrows=2)
        for field in fields:
            refused(rf"{who}: state\.{field} is null", fn, {k: v for k, v in st.items() if k != field})
    refused(r"mme_hierarchy_core: min_samples = 0", core, st, min_samples=0)
    refused(r"mme_hierarchy_core: min_samples = -3", core, st, min_samples=-3)
    for field in fields:
        refused(rf"mme_hierarchy_merge: state\.{field} is null", engine.hierarchy_merge, {k: v for k, v in st.items() if k != field})
    lib, h, S = engine.lib, engine.h, engine._hierarchy_struct(st)
    assert lib.mme_hierarchy_core(h, None, n, 128, None, 8, 0, n, S, None) == -1 and b"mme_hierarchy_core: emb is null" in lib.mme_last_error(h)
    assert lib.mme_hierarchy_scan(h, None, n, 128, None, 0, n, S, None) == -1 and b"mme_hierarchy_scan: emb is null" in lib.mme_last_error(h)
    assert lib.mme_hierarchy_scan(h, xb.data_ptr(), n, 128, None, 0, n, None, None) == -1 and b"mme_hierarchy_scan: state is null" in lib.mme_last_error(h)
    assert lib.mme_hierarchy_merge(h, None, n, None) == -1 and b"mme_hierarchy_merge: state is null" in lib.mme_last_error(h)
    assert lib.mme_hierarchy_init(h, S, -1, None) == -1 and b"mme_hierarchy_init: N = -1" in lib.mme_last_error(h)
    for field in fields:
        less = engine._hierarchy_struct({k: v for k, v in st.items() if k != field})
        assert lib.mme_hierarchy_init(h, less, n, None) == -1 and f"mme_hierarchy_init: state.{field} is null".encode() in lib.mme_last_error(h)
    odd = dict(st, core=st["core"].new_empty(n + 5)[1:])  # 4 bytes past a 16-byte boundary
    refused(r"mme_hierarchy_scan: state\.core = 0x[0-9a-f]+ is not 16-byte aligned", scan, odd)
    # nothing was enqueued: the same state and engine give the earlier result
    core(st)
    n_edges, rounds = engine.hierarchy_rounds(st, lambda: scan(st))
    edges, weights = engine.hierarchy_sorted(st, n_edges)
    after = _host({"edges": edges, "weights": weights, "core": st["core"][:n]})
    for k in ("edges", "weights", "core"):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert rounds == before["rounds"]


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
def _collection(x32, n_pages=12):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    n = len(x32)
    page = np.random.default_rng(11).integers(0, n_pages, n)
    col = RegionCollection()
    metas = [{"parent_image": f"/scans/issue{page[r] // 3:02d}_page{page[r]:02d}.png", "region_type": ["text", "figure", "advert"][r % 3],
              "area_percentage": float(1 + r % 17), "box_str": f"{r},{r + 1},{r + 40},{r + 60}", "is_region": True} for r in range(n)]
    ids = [f"region_{r:04d}" for r in range(n)]
    col.upsert(ids=ids + ["region_hole_a", "region_hole_b", "page_0"],
               embeddings=[x32[r].tolist() for r in range(n)] + [x32[0].tolist(), x32[1].tolist(), x32[0].tolist()],
               metadatas=metas + [dict(metas[0]), dict(metas[1]), {"is_region": False, "filename": "issue00_page00.png"}])
    col.update(ids=["region_hole_a", "region_hole_b"], embeddings=[None, []])  # two regions without an embedding: left out
    return col, ids, metas


def test_region_hierarchy_over_a_collection(engine, tmp_path):
    import json

    from multimodal_embeddings_amd import region_compare as rc
    from multimodal_embeddings_amd import store
    from multimodal_embeddings_amd.cross_compare import to_unit_bf16

    n, d = 203, 64
    col, ids, metas = _collection(R.table(n, d, 2)["x32"])
    x32 = to_unit_bf16([col.embeddings[r] for r in range(n)], engine).float().cpu().numpy()
    S = DR.similarity(x32)
    tau, gap = DR.widest_gap(S)
    assert gap >= 4 * DR.delta(d)
    summaries = set()
    for exclude in ("none", "parent", "prefix"):
        group = rc.duplicate_inputs(metas, exclude, prefix_length=7)[0]
        ref = R.reference(x32, tau, 8, group, S=S)
        assert DR.dead_zone_pairs(S, ref["adm"], tau, DR.delta(d)) == 0
        is_core = ref["kind"] == 2
        want = rc.density_table(np.where(is_core, ref["labels"], -1), np.where(is_core, 2, 0), ref["count"], np.full(n, -1), np.zeros(n), ids, metas,
                                threshold=tau, min_samples=8)
        for c in want["clusters"]:
            for m in c["members"]:
                del m["count"]
        h = rc.region_hierarchy(col, 8, exclude=exclude, prefix_length=7, engine=engine)
        assert h.ids == ids and h.components == 1 and len(h.edges) == n - 1 and h.rounds >= 2
        got = h.cut(tau)
        assert got == want and got["clusters"] and got["summary"]["n_core"] == int(is_core.sum())
        summaries.add(json.dumps(got["summary"]))
    assert len(summaries) == 3
    back = store.load_hierarchy(store.save_hierarchy(h, tmp_path / "tree"))
    assert back.edges.tobytes() == h.edges.tobytes() and back.weights.tobytes() == h.weights.tobytes() and back.ids == ids
    out = tmp_path / "reports" / "hierarchy.json"
    report = rc.create_hierarchy_report(col, 8, str(out), thresholds=(tau,), min_cluster_size=5, engine=engine)
    assert json.loads(out.read_text()) == report and len(report["edges"]) == n - 1 and len(report["clusters"]["clusters"]) >= 2


# ---- 9. streams ------------------------------------------------------------------------------------------------------------------
def _probe_inputs(v):
    t = R.table(331, 128, 1 + v)
    return {"emb": t["xb"], "group": torch.from_numpy(R.group_ids(331, 1 + v))}, {}


def _probe_setup():  # the cosine workspace grows on first use, which waits for the device: grown here, before the probe
    import stream_probes as sp
    from multimodal_embeddings_amd._lib import Engine

    eng = Engine(0)
    warm = sp.to_device(_probe_inputs(2)[0])
    eng.hierarchy(warm["emb"], 8, warm["group"])
    torch.cuda.synchronize()
    return eng


def test_the_one_shot_call_runs_on_the_caller_s_stream():
    """Probes A and B of tests/stream_probes.py over Engine.hierarchy: bit-equal to the default-stream run under both.  The
    one-shot call reads the edge counter back once per round, on its own stream; under probe A (the null stream busy, the call
    on a side stream) that wait does not touch the delay, and the probe must be effective.  Under probe B the delay sits on the
    call's own stream, so the first round's read-back waits it out by construction: what B can show for the one-shot call is the
    equality alone, and that the delay is still pending when it matters is asserted on the asynchronous entry points below."""
    import stream_probes as sp

    def call(eng, d, h):
        res = eng.hierarchy(d["emb"], 8, d["group"])
        return {k: res[k] for k in ("edges", "weights", "core")}

    case = sp.Case("hierarchy", "hierarchy-one-shot", _probe_setup, _probe_inputs, call)
    ref = sp.reference(case, 0)
    assert ref["edges"].shape == (330, 2) and not np.array_equal(ref["edges"], sp.reference(case, 1)["edges"])
    bad, effective = sp.probe_a(case)
    print(f"hierarchy probe A: the delay was {'still pending' if effective else 'over'} when it mattered")
    assert not bad and effective, bad
    bad, effective = sp.probe_b(case)
    print(f"hierarchy probe B: the delay was {'still pending' if effective else 'over'} when it mattered")
    assert not bad, bad


def test_the_asynchronous_entry_points_run_on_the_caller_s_stream():
    """init, core, and five rounds of scan and merge without any read-back (a round after the tree is whole emits nothing):
    probes A and B, both effective, bit-equal to the default-stream run."""
    import stream_probes as sp

    def call(eng, d, h):
        st = eng.hierarchy_init(331)
        eng.hierarchy_core(st, d["emb"], d["group"], min_samples=8)
        for _ in range(5):
            eng.hierarchy_scan(st, d["emb"], d["group"])
            eng.hierarchy_merge(st)
        return {k: st[k] for k in ("edges", "weights", "core", "counters", "comp")}

    def canon(got):  # the order in which a round's edges land is not specified
        order = np.lexsort((got["edges"][:, 1], got["edges"][:, 0], -got["weights"].astype(np.float64)))
        return {**got, "edges": got["edges"][order], "weights": got["weights"][order]}

    case = sp.Case("hierarchy_pieces", "hierarchy-init-core-scan-merge", _probe_setup, _probe_inputs, call, canon)
    ref = sp.reference(case, 0)
    assert ref["counters"].tolist() == [330, 5, 1] and (ref["comp"][:331] == 0).all()
    for name, probe in (("A", sp.probe_a), ("B", sp.probe_b)):
        bad, effective = probe(case)
        print(f"hierarchy pieces probe {name}: the delay was {'still pending' if effective else 'over'} when it mattered")
        assert not bad and effective, (name, bad, effective)
