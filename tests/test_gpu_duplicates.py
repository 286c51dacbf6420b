"""K14 near-duplicate groups (mme_duplicates_*, Engine.duplicates, region_compare.duplicate_groups) against the float64 /
scipy reference of tests/duplicates_reference.py.

Every case first asserts, on the reference alone, that no admissible pair lies in the dead zone [tau - delta, tau + delta)
of the contract: then labels, degrees, counts, page pairs and the edge set have exactly one right answer."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duplicates_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    return Engine(0)


def _host(res):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "edges" in out:
        w = int(out["counters"][1])
        out["edges"], out["edge_sim"] = out["edges"][:w], out["edge_sim"][:w]
    return out


def _edge_set(e):
    return sorted(map(tuple, np.asarray(e).reshape(-1, 2).tolist()))


def _check_fixture(ref, tau, d, adm=None):
    """the conditions under which the reference is the only right answer (a fixture error, never a skip)"""
    dead = R.dead_zone_pairs(ref["S"], ref["adm"] if adm is None else adm, tau, R.delta(d))
    assert dead == 0, f"fixture: {dead} admissible pairs inside the dead zone of tau = {tau}"
    assert ref["ambiguous"].sum() <= 0.01 * len(ref["labels"]), "fixture: more than 1 % of the rows have two best partners within 2 delta"


def _check_against(got, ref, d, cap_suffices=True):
    dl = R.delta(d)
    assert np.array_equal(got["labels"], ref["labels"]), np.flatnonzero(got["labels"] != ref["labels"])[:8]
    assert np.array_equal(got["degree"], ref["degree"]), np.flatnonzero(got["degree"] != ref["degree"])[:8]
    assert got["summary"].tolist() == ref["summary"].tolist()
    assert int(got["counters"][0]) == len(ref["edges"])
    err = np.abs(got["best_sim"].astype(np.float64) - ref["best_sim"])
    print(f"max |best_sim - ref| = {err.max() if len(err) else 0:.3e} (delta = {dl:.3e})")
    assert (err <= dl).all(), err.max()
    strict = ~ref["ambiguous"]
    assert np.array_equal(got["best_idx"][strict], ref["best_idx"][strict])
    for r in np.flatnonzero(ref["ambiguous"]):  # either of the two near-equal partners: an edge of the row within 2 delta of its best
        j = int(got["best_idx"][r])
        assert j >= 0 and ref["adm"][r, j] and ref["S"][r, j] >= ref["best_sim"][r] - 2 * dl
    if ref["page_pairs"] is not None:
        assert np.array_equal(got["page_pairs"], ref["page_pairs"])
    if "edges" in got and cap_suffices:
        assert int(got["counters"][1]) == len(ref["edges"])
        assert _edge_set(got["edges"]) == _edge_set(ref["edges"])
        order = np.lexsort((got["edges"][:, 1], got["edges"][:, 0]))
        want = ref["S"][ref["edges"][:, 0], ref["edges"][:, 1]]
        assert (np.abs(got["edge_sim"][order].astype(np.float64) - want) <= dl).all()


def _run(engine, c, cap=0, **kw):
    xb = c["xb"].cuda()
    return _host(engine.duplicates(xb, c["group"], c["group"], c["pages"], min_sim=c["tau"], edge_cap=cap, **kw))


@pytest.mark.parametrize("n,d,pages", [(n, d, 0) for n, d in R.SHAPES] + [(331, 128, 12), (515, 768, 12)])
def test_whole_run_matches_reference(engine, n, d, pages):
    c = R.case(n, d, 1, pages)
    assert c["gap"] >= 4 * R.delta(d), c["gap"] / R.delta(d)
    _check_fixture(c["ref"], c["tau"], d)
    got = _run(engine, c, cap=len(c["ref"]["edges"]) + 7)
    _check_against(got, c["ref"], d)
    if pages:
        assert np.array_equal(got["page_pairs"], got["page_pairs"].T) and np.trace(got["page_pairs"]) == 0


_KEYS = ("labels", "degree", "best_idx", "best_sim", "summary", "counters")


def _same(a, b, keys=_KEYS):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint8) if b[k].dtype == np.float32 else b[k]), k


def test_row_shards_accumulate_into_one_state(engine):
    """Shards in any order are one run; the ranges start at rows 37 and 38, so the first useful column of a block is no
    multiple of 4 past its first column, and nrows = 0 does nothing."""
    c = R.case(515, 256, 1)
    _check_fixture(c["ref"], c["tau"], 256)
    cap = len(c["ref"]["edges"]) + 3
    whole = _run(engine, c, cap=cap)
    _check_against(whole, c["ref"], 256)
    xb = c["xb"].cuda()
    st = engine.duplicates_init(515, edge_cap=cap)
    for row0, nrows in [(300, 215), (37, 1), (100, 0), (0, 37), (515, 0), (38, 262)]:
        engine.duplicates_scan(st, xb, min_sim=c["tau"], row0=row0, nrows=nrows)
    got = _host(engine.duplicates_finish(st))
    _same(got, whole)
    assert _edge_set(got["edges"]) == _edge_set(whole["edges"])


def test_merge_of_two_states_equals_one_run(engine):
    c = R.case(515, 256, 1, 0)
    pages = 9
    page = (np.arange(515) % pages).astype(np.int32)
    ref = R.reference(c["x32"], c["tau"], page, page, pages)
    _check_fixture(ref, c["tau"], 256)
    xb = c["xb"].cuda()
    whole = _host(engine.duplicates(xb, page, page, pages, min_sim=c["tau"]))
    _check_against(whole, ref, 256)
    A, B = engine.duplicates_init(515, pages=pages), engine.duplicates_init(515, pages=pages)
    for r in range(515):
        engine.duplicates_scan(B if r % 2 else A, xb, page, page, min_sim=c["tau"], row0=r, nrows=1)
    engine.duplicates_merge(A, B)
    got = _host(engine.duplicates_finish(A))
    _same(got, whole)
    assert np.array_equal(got["page_pairs"], whole["page_pairs"])


@pytest.mark.parametrize("permuted", [False, True])
def test_chain_is_one_component(engine, permuted):
    """x_i = (e_i + e_{i+1}) / sqrt 2: adjacent rows at cosine 0.49989 (the square of bf16(1 / sqrt 2)), all others 0: a path
    of N rows, the deepest tree the hooks can build."""
    n, d = 1000, 1024
    x = np.zeros((n, d), dtype=np.float32)
    x[np.arange(n), np.arange(n)] = 2 ** -0.5
    x[np.arange(n), np.arange(n) + 1] = 2 ** -0.5
    perm = np.random.default_rng(5).permutation(n) if permuted else np.arange(n)
    x = x[perm]
    x32, xb = R.to_bf16(x)
    S = R.similarity(x32)
    off = S[np.triu_indices(n, 1)]
    assert set(np.round(off, 5).tolist()) == {0.0, 0.49989} and R.dead_zone_pairs(S, R.admissible(n), 0.3, R.delta(d)) == 0
    got = _host(engine.duplicates(xb.cuda(), min_sim=0.3))
    assert (got["labels"] == 0).all()
    assert int(got["counters"][0]) == n - 1 and got["summary"].tolist() == [n - 1, 1, n, n]
    inv = np.argsort(perm)  # position of chain element k
    want = np.full(n, 2)
    want[inv[0]] = want[inv[n - 1]] = 1
    assert np.array_equal(got["degree"], want)


def test_one_root_under_contention(engine):
    """500 identical rows: every pair is the same sum of the same products, so the f32 values are bit-equal and the tie rule
    alone decides the best partner; every union lands on one root."""
    n, d = 500, 64
    v = np.random.default_rng(3).standard_normal(d)
    x32, xb = R.to_bf16(np.tile(v / np.linalg.norm(v), (n, 1)))
    xb = xb.cuda()
    got = _host(engine.duplicates(xb, min_sim=0.5, edge_cap=n * (n - 1) // 2))
    assert int(got["counters"][0]) == int(got["counters"][1]) == 124750 and got["summary"].tolist() == [124750, 1, n, n]
    assert (got["labels"] == 0).all() and (got["degree"] == n - 1).all()
    assert len(set(got["best_sim"].view(np.uint32).tolist())) == 1 and len(set(got["edge_sim"].view(np.uint32).tolist())) == 1
    assert got["best_idx"].tolist() == [1] + [0] * (n - 1)
    assert _edge_set(got["edges"]) == [(i, j) for i in range(n) for j in range(i + 1, n)]
    got = _host(engine.duplicates(xb, np.arange(n, dtype=np.int32) % 2, min_sim=0.5))
    assert int(got["counters"][0]) == 62500 and got["summary"].tolist() == [62500, 1, n, n]
    assert (got["labels"] == 0).all() and (got["degree"] == n // 2).all()
    assert got["best_idx"].tolist() == [1, 0] * (n // 2)


@pytest.mark.parametrize("n", [1, 2, 5, 203])
def test_empty_answer_and_tiny_tables(engine, n):
    x32, xb = R.walks(n, 64, 7)
    got = _host(engine.duplicates(xb.cuda(), min_sim=1.5, edge_cap=4))
    assert got["labels"].tolist() == list(range(n)) and (got["degree"] == 0).all()
    assert (got["best_idx"] == -1).all() and (got["best_sim"] == 0).all()
    assert got["summary"].tolist() == [0, 0, 0, 0] and got["counters"].tolist() == [0, 0] and len(got["edges"]) == 0
    if n <= 5:  # and a threshold everything passes: one group
        tau = -1.5
        ref = R.reference(x32, tau)
        _check_fixture(ref, tau, 64)
        _check_against(_host(engine.duplicates(xb.cuda(), min_sim=tau, edge_cap=16)), ref, 64)


def test_edge_cap_truncates_to_a_valid_subset(engine):
    c = R.case(331, 128, 1)
    _check_fixture(c["ref"], c["tau"], 128)
    assert len(c["ref"]["edges"]) > 50
    got = _run(engine, c, cap=50)
    assert int(got["counters"][0]) == len(c["ref"]["edges"]) and int(got["counters"][1]) == 50 and len(got["edges"]) == 50
    pairs = _edge_set(got["edges"])
    assert len(set(pairs)) == 50 and all(i < j for i, j in pairs)
    assert set(pairs) <= set(_edge_set(c["ref"]["edges"]))
    _check_against(got, c["ref"], 128, cap_suffices=False)


def test_across_the_workspace_chunks(engine):
    """N = 40 000 rows of 61 classes x_i = e_(i mod 61): 6.4 GB of cosine values, so several chunks of at most 2 GiB, each
    starting at another column; the answer is known without an N^2 reference."""
    n, d, k = 40000, 64, 61
    cls = torch.arange(n, device="cuda") % k
    xb = torch.zeros((n, d), dtype=torch.bfloat16, device="cuda")
    xb[torch.arange(n, device="cuda"), cls] = 1.0
    got = _host(engine.duplicates(xb, min_sim=0.5))
    size = np.bincount(np.arange(n) % k)
    assert size.max() == 656
    assert np.array_equal(got["labels"], np.arange(n) % k)
    assert np.array_equal(got["degree"], size[np.arange(n) % k] - 1)
    edges = int((size * (size - 1) // 2).sum())
    assert int(got["counters"][0]) == edges and got["summary"].tolist() == [edges, k, n, 656]
    want = np.where(np.arange(n) < k, np.arange(n) + k, np.arange(n) % k)  # all values are exactly 1: the lowest partner
    assert np.array_equal(got["best_idx"], want) and (got["best_sim"] == 1.0).all()


def test_two_runs_are_bit_equal(engine):
    c = R.case(515, 768, 1, 12)
    a, b = _run(engine, c), _run(engine, c)
    _same(a, b)
    assert np.array_equal(a["page_pairs"], b["page_pairs"])


def test_refusals_name_the_field_and_leave_the_state_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError

    c = R.case(331, 128, 1, 12)
    _check_fixture(c["ref"], c["tau"], 128)
    xb, g = c["xb"].cuda(), torch.from_numpy(c["group"]).cuda()
    n = 331
    before = _run(engine, c)
    st = engine.duplicates_init(n, pages=12)
    scan = lambda state, emb=xb, page_of=g, **kw: engine.duplicates_scan(state, emb, g, page_of, **{"min_sim": c["tau"], **kw})  # noqa: E731

    def refused(match, fn, *a, **kw):
        with pytest.raises(MmeError, match=match):
            fn(*a, **kw)

    refused(r"d = 96", scan, dict(st), emb=torch.zeros((n, 96), dtype=torch.bfloat16, device="cuda"))
    refused(r"rows \[row0 = 300, row0 \+ nrows = 332\)", scan, st, row0=300, nrows=32)
    refused(r"rows \[row0 = -1", scan, st, row0=-1, nrows=2)
    refused(r"page_of is null", scan, st, page_of=None)
    refused(r"state\.P = 4097", scan, {**st, "pages": 4097})
    refused(r"state\.P = 0", scan, {**st, "pages": 0})
    refused(r"min_sim is NaN", scan, st, min_sim=float("nan"))
    refused(r"edge_cap = -1", scan, {**st, "edge_cap": -1})
    refused(r"edges is null with edge_cap = 8", scan, {**st, "edge_cap": 8})
    for field in ("parent", "degree", "best", "counters"):
        refused(rf"state\.{field} is null", scan, {k: v for k, v in st.items() if k != field})
        refused(rf"state\.{field} is null", engine.duplicates_finish, {k: v for k, v in st.items() if k != field})
    refused(r"src\.parent is null", engine.duplicates_merge, st, {k: v for k, v in st.items() if k != "parent"})
    refused(r"page_pairs of dst \(P = 12\) and src \(P = 0\)", engine.duplicates_merge, st, engine.duplicates_init(n))
    rc = engine.lib.mme_duplicates_scan(engine.h, None, n, 128, None, g.data_ptr(), 0.5, 0, n, engine._dup_struct(st), None)
    assert rc == -1 and b"emb is null" in engine.lib.mme_last_error(engine.h)
    rc = engine.lib.mme_duplicates_scan(engine.h, xb.data_ptr(), n, 128, None, g.data_ptr(), 0.5, 0, n, None, None)
    assert rc == -1 and b"state is null" in engine.lib.mme_last_error(engine.h)
    # nothing was enqueued: the same state and engine give the earlier result
    scan(st)
    _same(_host(engine.duplicates_finish(st)), before)


HOLES = ("region_hole_a", "region_hole_b")


def _collection(x32, n_pages=12):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    n = len(x32)
    rng = np.random.default_rng(11)
    page = rng.integers(0, n_pages, n)
    col = RegionCollection()
    metas = [{"parent_image": f"/scans/issue{page[r] // 3:02d}_page{page[r]:02d}.png", "region_type": ["text", "figure", "advert"][r % 3],
              "area_percentage": float(1 + r % 17), "box_str": f"{r},{r + 1},{r + 40},{r + 60}", "is_region": True} for r in range(n)]
    embs = [x32[r].tolist() for r in range(n)]
    ids = [f"region_{r:04d}" for r in range(n)]
    # two more regions (the test takes their embeddings away), and a page row that is no region
    ids += list(HOLES) + ["page_0"]
    embs += [x32[0].tolist(), x32[1].tolist(), x32[0].tolist()]
    metas += [dict(metas[0]), dict(metas[1]), {"is_region": False, "filename": "issue00_page00.png"}]
    col.upsert(ids=ids, embeddings=embs, metadatas=metas)
    return col, ids[:n], metas[:n]


def _assert_reports_equal(a, b, tol):
    """equal documents, the scores within `tol`"""
    assert type(a) is type(b), (a, b)
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            if k == "score":
                assert abs(a[k] - b[k]) <= tol
            else:
                _assert_reports_equal(a[k], b[k], tol)
    elif isinstance(a, list):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            _assert_reports_equal(u, v, tol)
    else:
        assert a == b


def test_duplicate_groups_over_a_collection(engine, tmp_path):
    from multimodal_embeddings_amd import region_compare as rc
    from multimodal_embeddings_amd.cross_compare import to_unit_bf16

    n, d = 331, 128
    col, ids, metas = _collection(R.case(n, d, 1)["x32"])
    neighbours_before = rc.region_neighbours(col, 5, engine=engine)
    held = [col.embeddings[col._pos[i]] for i in HOLES]
    col.update(ids=list(HOLES), embeddings=[None, []])  # two regions without an embedding: left out, as `query` leaves them out
    # the table the collection's rows become on the device: L2-normalised again, rounded to bf16
    x32 = to_unit_bf16([col.embeddings[r] for r in range(n)], engine).float().cpu().numpy()
    tau, gap = R.widest_gap(R.similarity(x32))
    assert gap >= 4 * R.delta(d)
    for exclude in ("parent", "prefix", "none"):
        group, page_of, names = rc.duplicate_inputs(metas, exclude, prefix_length=7)
        assert len(names) == 12 and (group is None) == (exclude == "none")
        ref = R.reference(x32, tau, group, page_of, len(names))
        _check_fixture(ref, tau, d)
        assert not ref["ambiguous"].any()
        want = rc.group_table(ref["labels"], ref["degree"], ref["best_idx"], ref["best_sim"], ids, metas, threshold=tau, page_pairs=ref["page_pairs"],
                              image_names=names, edges=ref["edges"], edge_sim=ref["S"][ref["edges"][:, 0], ref["edges"][:, 1]],
                              n_edges=len(ref["edges"]))
        got = rc.duplicate_groups(col, tau, exclude=exclude, prefix_length=7, max_edges=1000, engine=engine)
        _assert_reports_equal(got, want, R.delta(d))
        assert got["n_regions"] == n and got["groups"] and not got["edges"]["truncated"]
    assert len({len(R.reference(x32, tau, rc.duplicate_inputs(metas, e, 7)[0])["edges"]) for e in ("parent", "prefix", "none")}) == 3
    out = tmp_path / "reports" / "duplicates.json"
    report = rc.create_duplicate_report(col, tau, str(out), exclude="prefix", prefix_length=7, max_edges=20)
    assert report["edges"]["truncated"] and len(report["edges"]["pairs"]) == 20
    assert json.loads(out.read_text()) == report
    col.update(ids=list(HOLES), embeddings=held)
    assert rc.region_neighbours(col, 5, engine=engine) == neighbours_before
