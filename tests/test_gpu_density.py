"""K18 density clusters (mme_density_*, Engine.density_*, region_compare.density_clusters / kth_neighbour_similarity) against the
float64 / scipy reference of tests/density_reference.py.

Every case first asserts, on the reference alone, the conditions under which it is the only right answer (no admissible pair
in the dead zone of the threshold, a gap of 4 delta, no border row between two clusters within 2 delta); then labels, kind,
count and summary are compared exactly, border_sim within delta, border_idx exactly except on the rows whose two best core
neighbours lie within 2 delta."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as R  # noqa: E402
import duplicates_reference as DR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    return Engine(0)


def _host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_against(got, ref, d):
    dl = DR.delta(d)
    for k in ("count", "kind", "labels"):
        assert np.array_equal(got[k], ref[k]), (k, np.flatnonzero(got[k] != ref[k])[:8])
    assert got["summary"].tolist() == ref["summary"].tolist()
    assert got["counters"].tolist() == [int(ref["summary"][0])] * 2  # both passes saw the same pairs
    err = np.abs(got["border_sim"].astype(np.float64) - ref["border_sim"])
    print(f"max |border_sim - ref| = {err.max() if len(err) else 0:.3e} (delta = {dl:.3e})")
    assert (err <= dl).all(), err.max()
    strict = ~ref["idx_ties"]
    assert np.array_equal(got["border_idx"][strict], ref["border_idx"][strict])
    for r in np.flatnonzero(ref["idx_ties"]):  # either of the near-equal partners: a core neighbour within 2 delta of the best
        j = int(got["border_idx"][r])
        assert j >= 0 and ref["kind"][j] == 2 and ref["adm"][r, j] and ref["S"][r, j] >= ref["border_sim"][r] - 2 * dl


def _run(engine, c, min_samples=None):
    return _host(engine.density_clusters(c["xb"].cuda(), c["tau"], c["min_samples"] if min_samples is None else min_samples, c["group"]))


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("min_samples", [3, 8])
@pytest.mark.parametrize("n,d,seed", R.CASES)
def test_whole_run_matches_reference(engine, n, d, seed, min_samples, grouped):
    c = R.case(n, d, seed, min_samples, grouped)
    R.check_fixture(c)
    _check_against(_run(engine, c), c["ref"], d)


_KEYS = ("labels", "kind", "count", "border_idx", "border_sim", "summary", "counters")


def _same(a, b, keys=_KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape, k


def test_row_shards_count_in_any_order_and_link_in_another_split(engine):
    """The count ranges start at rows 37 and 38 (the first useful column of a block is no multiple of 4 past its first column)
    and at 300 (past the first 256-row tile); the link pass takes another split: a pair's f32 value, and so the edge set of
    the two passes, must not depend on the chunk the pair falls in."""
    c = R.case(515, 256, 1, 8)
    R.check_fixture(c)
    whole = _run(engine, c)
    _check_against(whole, c["ref"], 256)
    xb = c["xb"].cuda()
    st = engine.density_init(515)
    for row0, nrows in [(300, 215), (37, 1), (100, 0), (0, 37), (515, 0), (38, 262)]:
        engine.density_count(st, xb, min_sim=c["tau"], row0=row0, nrows=nrows)
    for row0, nrows in [(0, 200), (200, 315)]:
        engine.density_link(st, xb, min_sim=c["tau"], min_samples=8, row0=row0, nrows=nrows)
    _same(_host(engine.density_finish(st, min_samples=8)), whole)


@pytest.mark.parametrize("grouped", [False, True])
def test_min_samples_1_and_2_are_k14(engine, grouped):
    c = R.case(331, 128, 1, 8, grouped)  # K14 leaves 5 singletons here
    R.check_fixture(c)
    xb = c["xb"].cuda()
    k14 = {k: v.cpu().numpy() for k, v in engine.duplicates(xb, c["group"], min_sim=c["tau"]).items()}
    one = _run(engine, c, 1)
    assert np.array_equal(one["labels"], k14["labels"]) and np.array_equal(one["count"], k14["degree"]) and (one["kind"] == 2).all()
    assert (one["border_idx"] == -1).all() and (one["border_sim"] == 0).all()
    sizes = np.bincount(k14["labels"], minlength=331)
    assert one["summary"].tolist() == [int(k14["counters"][0]), int((sizes > 0).sum()), 331, 0, 0, int(sizes.max())]
    two = _run(engine, c, 2)
    single = sizes[k14["labels"]] == 1
    assert np.array_equal(two["labels"], np.where(single, -1, k14["labels"])) and np.array_equal(two["kind"], np.where(single, 0, 2))
    assert two["summary"].tolist() == [int(k14["summary"][0]), int(k14["summary"][1]), int(k14["summary"][2]), 0, int(single.sum()), int(k14["summary"][3])]
    assert single.any() and not single.all()


def test_one_root_under_contention(engine):
    """500 identical rows: at min_samples = 500 every row is core (499 neighbours and itself) and every union lands on one
    root; at 501 no row is."""
    n, d = 500, 64
    v = np.random.default_rng(3).standard_normal(d)
    xb = DR.to_bf16(np.tile(v / np.linalg.norm(v), (n, 1)))[1].cuda()
    got = _host(engine.density_clusters(xb, 0.5, 500))
    assert (got["labels"] == 0).all() and (got["kind"] == 2).all() and (got["count"] == n - 1).all()
    assert got["summary"].tolist() == [124750, 1, n, 0, 0, n] and got["counters"].tolist() == [124750, 124750]
    got = _host(engine.density_clusters(xb, 0.5, 501))
    assert (got["labels"] == -1).all() and (got["kind"] == 0).all() and (got["count"] == n - 1).all()
    assert (got["border_idx"] == -1).all() and (got["border_sim"] == 0).all()
    assert got["summary"].tolist() == [124750, 0, 0, 0, n, 0]


def star(d=64):
    """a centre row c and 12 rows normalise(c + 0.75 e_k): cosine 0.8 to the centre, 0.64 to each other"""
    x = np.zeros((13, d))
    x[:, 0] = 1.0
    x[np.arange(1, 13), np.arange(1, 13)] = 0.75
    return DR.to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


@pytest.mark.parametrize("permuted", [False, True])
def test_a_star_has_one_core_and_twelve_border_rows(engine, permuted):
    x32, xb = star()
    if permuted:  # the centre in the middle: border rows on both sides of their core row
        perm = np.random.default_rng(4).permutation(13)
        x32, xb = x32[perm], xb[torch.from_numpy(perm)]
    tau = 0.7
    centre = int(np.flatnonzero(x32[:, 1:].max(1) == 0)[0])
    for min_samples, want in ((13, [12, 1, 1, 12, 0, 13]), (14, [12, 0, 0, 0, 13, 0])):
        ref = R.reference(x32, tau, min_samples)
        assert DR.dead_zone_pairs(ref["S"], ref["adm"], tau, DR.delta(64)) == 0 and not ref["ambiguous"].any() and not ref["idx_ties"].any()
        assert ref["summary"].tolist() == want
        got = _host(engine.density_clusters(xb.cuda(), tau, min_samples))
        _check_against(got, ref, 64)
        if min_samples == 13:
            assert (got["labels"] == centre).all() and got["kind"][centre] == 2 and (np.delete(got["border_idx"], centre) == centre).all()


@pytest.mark.parametrize("n", [1, 2, 5])
def test_tiny_tables_empty_answers_and_min_samples_beyond_n(engine, n):
    x32, xb = R.blobs(n, 64, 7)
    xb = xb.cuda()
    # a threshold nothing passes: all noise at min_samples = 2, all core singletons at 1
    got = _host(engine.density_clusters(xb, 1.5, 2))
    assert (got["labels"] == -1).all() and (got["kind"] == 0).all() and (got["count"] == 0).all()
    assert got["summary"].tolist() == [0, 0, 0, 0, n, 0] and got["counters"].tolist() == [0, 0]
    got = _host(engine.density_clusters(xb, 1.5, 1))
    assert got["labels"].tolist() == list(range(n)) and (got["kind"] == 2).all() and got["summary"].tolist() == [0, n, n, 0, 0, 1]
    assert (got["border_idx"] == -1).all() and (got["border_sim"] == 0).all()
    # a threshold everything passes: one cluster up to min_samples = n, noise beyond
    tau = -1.5
    for min_samples in (1, n, n + 1, 2 ** 31 - 1):
        ref = R.reference(x32, tau, min_samples)
        assert DR.dead_zone_pairs(ref["S"], ref["adm"], tau, DR.delta(64)) == 0
        assert ref["summary"].tolist() == ([n * (n - 1) // 2, 1, n, 0, 0, n] if min_samples <= n else [n * (n - 1) // 2, 0, 0, 0, n, 0])
        _check_against(_host(engine.density_clusters(xb, tau, min_samples)), ref, 64)


def test_min_samples_beyond_every_count(engine):
    c = R.case(203, 64, 1, 8)
    most = int(c["ref"]["count"].max()) + 1
    assert 8 < most < 203
    for min_samples, cores in ((most, True), (most + 1, False), (204, False)):
        ref = R.reference(c["x32"], c["tau"], min_samples, S=c["S"])
        assert bool(ref["summary"][2]) == cores and not ref["ambiguous"].any()
        got = _run(engine, c, min_samples)
        _check_against(got, ref, 64)
    assert (got["labels"] == -1).all() and got["summary"].tolist()[1:] == [0, 0, 0, 203, 0]


def test_across_the_workspace_chunks(engine):
    """N = 40 000 rows of 61 classes x_i = e_(i mod 61): 6.4 GB of cosine values per pass, so several chunks of at most 2 GiB,
    each starting at another column.  45 classes have 656 rows, 16 have 655: at min_samples = 656 the former are 45 clusters of
    core rows, the latter 10 480 noise rows, known without an N^2 reference."""
    n, d, k = 40000, 64, 61
    cls = torch.arange(n, device="cuda") % k
    xb = torch.zeros((n, d), dtype=torch.bfloat16, device="cuda")
    xb[torch.arange(n, device="cuda"), cls] = 1.0
    got = _host(engine.density_clusters(xb, 0.5, 656))
    size = np.bincount(np.arange(n) % k)
    assert (size[:45] == 656).all() and (size[45:] == 655).all()
    c = np.arange(n) % k
    assert np.array_equal(got["count"], size[c] - 1)
    assert np.array_equal(got["labels"], np.where(c < 45, c, -1)) and np.array_equal(got["kind"], np.where(c < 45, 2, 0))
    assert (got["border_idx"] == -1).all() and (got["border_sim"] == 0).all()
    pairs = int((size * (size - 1) // 2).sum())
    assert pairs == 45 * 214840 + 16 * 214185
    assert got["summary"].tolist() == [pairs, 45, 29520, 0, 10480, 656] and got["counters"].tolist() == [pairs, pairs]


def test_two_runs_are_bit_equal(engine):
    c = R.case(515, 768, 1, 8, True)
    a, b = _run(engine, c), _run(engine, c)
    _same(a, b)
    assert (a["kind"] == 1).sum() > 20


def test_refusals_name_the_field_and_leave_the_state_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError

    c = R.case(331, 128, 1, 8, True)
    R.check_fixture(c)
    n, tau = 331, c["tau"]
    xb, g = c["xb"].cuda(), torch.from_numpy(c["group"]).cuda()
    before = _run(engine, c)
    st = engine.density_init(n)
    count = lambda state, emb=xb, **kw: engine.density_count(state, emb, g, **{"min_sim": tau, **kw})  # noqa: E731
    link = lambda state, emb=xb, **kw: engine.density_link(state, emb, g, **{"min_sim": tau, "min_samples": 8, **kw})  # noqa: E731

    def refused(match, fn, *a, **kw):
        with pytest.raises(MmeError, match=match):
            fn(*a, **kw)

    for who, fn in (("mme_density_count", count), ("mme_density_link", link)):
        refused(rf"{who}: d = 96", fn, st, emb=torch.zeros((n, 96), dtype=torch.bfloat16, device="cuda"))
        refused(rf"{who}: rows \[row0 = 300, row0 \+ nrows = 332\)", fn, st, row0=300, nrows=32)
        refused(rf"{who}: rows \[row0 = -1", fn, st, row0=-1, nrows=2)
        refused(rf"{who}: min_sim is NaN", fn, st, min_sim=float("nan"))
        for field in ("count", "parent", "border", "counters"):
            refused(rf"{who}: state\.{field} is null", fn, {k: v for k, v in st.items() if k != field})
    refused(r"mme_density_link: min_samples = 0", link, st, min_samples=0)
    refused(r"mme_density_link: min_samples = -3", link, st, min_samples=-3)
    refused(r"mme_density_finish: min_samples = 0", engine.density_finish, st, min_samples=0)
    for field in ("count", "parent", "border", "counters"):
        refused(rf"mme_density_finish: state\.{field} is null", engine.density_finish, {k: v for k, v in st.items() if k != field}, min_samples=8)
    lib, h, S = engine.lib, engine.h, engine._density_struct(st)
    out = {k: torch.empty(n, dtype=torch.float32 if k == "border_sim" else torch.int32, device="cuda") for k in ("labels", "kind", "border_idx", "border_sim")}
    summary = torch.empty(6, dtype=torch.int64, device="cuda")
    ptrs = [out[k].data_ptr() for k in ("labels", "kind", "border_idx", "border_sim")] + [summary.data_ptr()]
    for i, name in enumerate(("labels", "kind", "border_idx", "border_sim", "summary")):
        args = list(ptrs)
        args[i] = None
        assert lib.mme_density_finish(h, S, n, 8, *args, None) == -1 and f"mme_density_finish: {name} is null".encode() in lib.mme_last_error(h)
    assert lib.mme_density_count(h, None, n, 128, None, 0.5, 0, n, S, None) == -1 and b"mme_density_count: emb is null" in lib.mme_last_error(h)
    assert lib.mme_density_link(h, None, n, 128, None, 0.5, 8, 0, n, S, None) == -1 and b"mme_density_link: emb is null" in lib.mme_last_error(h)
    assert lib.mme_density_count(h, xb.data_ptr(), n, 128, None, 0.5, 0, n, None, None) == -1 and b"mme_density_count: state is null" in lib.mme_last_error(h)
    assert lib.mme_density_init(h, S, -1, None) == -1 and b"mme_density_init: N = -1" in lib.mme_last_error(h)
    for field in ("count", "parent", "border", "counters"):
        less = engine._density_struct({k: v for k, v in st.items() if k != field})
        assert lib.mme_density_init(h, less, n, None) == -1 and f"mme_density_init: state.{field} is null".encode() in lib.mme_last_error(h)
    # nothing was enqueued: the same state and engine give the earlier result
    count(st)
    link(st)
    _same(_host(engine.density_finish(st, min_samples=8)), before)


HOLES = ("region_hole_a", "region_hole_b")


def _collection(x32, n_pages=12):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    n = len(x32)
    page = np.random.default_rng(11).integers(0, n_pages, n)
    col = RegionCollection()
    metas = [{"parent_image": f"/scans/issue{page[r] // 3:02d}_page{page[r]:02d}.png", "region_type": ["text", "figure", "advert"][r % 3],
              "area_percentage": float(1 + r % 17), "box_str": f"{r},{r + 1},{r + 40},{r + 60}", "is_region": True} for r in range(n)]
    ids = [f"region_{r:04d}" for r in range(n)]
    col.upsert(ids=ids + list(HOLES) + ["page_0"], embeddings=[x32[r].tolist() for r in range(n)] + [x32[0].tolist(), x32[1].tolist(), x32[0].tolist()],
               metadatas=metas + [dict(metas[0]), dict(metas[1]), {"is_region": False, "filename": "issue00_page00.png"}])
    col.update(ids=list(HOLES), embeddings=[None, []])  # two regions without an embedding: left out
    return col, ids, metas


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


def test_density_clusters_and_the_knee_curve_over_a_collection(engine, tmp_path):
    from multimodal_embeddings_amd import region_compare as rc
    from multimodal_embeddings_amd.cross_compare import to_unit_bf16

    n, d = 203, 64
    col, ids, metas = _collection(R.table(n, d, 2)["x32"])
    # the table the collection's rows become on the device: L2-normalised again, rounded to bf16
    x32 = to_unit_bf16([col.embeddings[r] for r in range(n)], engine).float().cpu().numpy()
    S = DR.similarity(x32)
    tau, gap = DR.widest_gap(S)
    assert gap >= 4 * DR.delta(d)
    summaries = set()
    for exclude in ("none", "parent", "prefix"):
        group = rc.duplicate_inputs(metas, exclude, prefix_length=7)[0]
        assert (group is None) == (exclude == "none")
        ref = R.reference(x32, tau, 8, group, S=S)
        assert DR.dead_zone_pairs(S, ref["adm"], tau, DR.delta(d)) == 0 and not ref["ambiguous"].any() and not ref["idx_ties"].any()
        assert (ref["summary"][1:5] > 0).all()
        want = rc.density_table(ref["labels"], ref["kind"], ref["count"], ref["border_idx"], ref["border_sim"], ids, metas, threshold=tau, min_samples=8)
        got = rc.density_clusters(col, tau, 8, exclude=exclude, prefix_length=7, engine=engine)
        _assert_reports_equal(got, want, DR.delta(d))
        assert got["n_regions"] == n and got["clusters"] and got["noise"]["count"] == ref["summary"][4]
        summaries.add(json.dumps(got["summary"]))
    assert len(summaries) == 3
    out = tmp_path / "reports" / "density.json"
    report = rc.create_density_report(col, tau, 8, str(out), min_size=12, engine=engine)
    assert json.loads(out.read_text()) == report and report["clusters"] and all(c["size"] >= 12 for c in report["clusters"])
    # the knee curve from one K12 pass
    for exclude, k in (("none", 1), ("none", 7), ("parent", 7)):
        group = rc.duplicate_inputs(metas, exclude)[0]
        Sa = np.where(DR.admissible(n, group), S, -np.inf)
        want = np.sort(-np.sort(-Sa, axis=1)[:, k - 1])[::-1]
        got = rc.kth_neighbour_similarity(col, k, exclude=exclude, engine=engine)
        assert got.dtype == np.float32 and got.shape == (n,) and (np.diff(got) <= 0).all()
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"k = {k}, exclude = {exclude}: max |curve - ref| = {err:.3e} (delta = {DR.delta(d):.3e})")
        assert err <= DR.delta(d)


def test_the_one_shot_call_runs_on_the_caller_s_stream():
    """Probes A and B of tests/stream_probes.py, as tests/test_gpu_streams.py runs them for K14: the null stream busy and the
    call on a side stream, then a late input and two calls back to back; both bit-equal to the default-stream run."""
    import stream_probes as sp
    from multimodal_embeddings_amd._lib import Engine

    def inputs(v):
        t = R.table(331, 128, 1 + v)
        return {"emb": t["xb"], "group": torch.from_numpy(R.group_ids(331, 1 + v))}, {"tau": np.array([t["tau"]])}

    def setup():  # the cosine workspace grows on first use, which waits for the device: grown here, before the probe
        eng = Engine(0)
        warm = sp.to_device(inputs(2)[0])
        eng.density_clusters(warm["emb"], 0.5, 8, warm["group"])
        torch.cuda.synchronize()
        return eng

    def call(eng, d, h):
        return eng.density_clusters(d["emb"], float(h["tau"][0]), 8, d["group"])

    case = sp.Case("density_clusters", "density-init-count-link-finish", setup, inputs, call)
    ref = sp.reference(case, 0)
    assert (ref["kind"] == 1).any() and (ref["kind"] == 2).any() and (ref["kind"] == 0).any()
    effective = {}
    for name, probe in (("A", sp.probe_a), ("B", sp.probe_b)):
        bad, effective[name] = probe(case)
        print(f"density_clusters probe {name}: the delay was {'still pending' if effective[name] else 'over'} when it mattered")
        assert not bad, (name, bad)
    assert any(effective.values()), "no effective probe"
