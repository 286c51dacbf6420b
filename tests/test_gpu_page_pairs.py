"""K10, the page-pair reduction (pick_queries -> cosine GEMM -> page_pairs -> normalise), against oracle.compare on inputs
whose expected output is exact (tests/page_pairs_reference.py).

Reference: oracle.compare.compute_image_similarity_matrix / pair_terms in float64, fed with cosines computed on the HOST
as e64 @ e64.T from the bf16 rows -- not with the device's GEMM, so the comparison is independent of the device.

Why it is exact (np.array_equal, raw and normalised, both metrics).  Rows have entries in {0, +-1/8}: every dot product is
a multiple of 1/64 with sum |a b| < 2^24 / 64 (asserted), exact in f32 in any accumulation order, so the device's cosines
are the float64 ones and every top-k, tie and threshold decision is made on identical numbers.  area_percentage is
100 / 2^k or 0: area / 100 is a power of two, each term a multiple of 2^-18 below 2, and a sum of at most 128 terms exact
in f64 in any order.  The normalised form adds one IEEE division per entry.  One case keeps generic areas, where the
result depends on numpy's pairwise order that the kernel restates: the project's 1e-15 absolute bound applies there.

One table of 12 pages with 300, 7, 256, 257, 64, 65, 1, 130, 0, 40, 12 and 300 rows (the register path at each register's
edge, the general path, an empty and a one-row page), d = 64 and d = 128, runs of exact duplicates inside and across
pages.  Grid (max_query, top_k, threshold): page_pairs_reference.GRID, the limit max_query * top_k = 128 both ways round;
thresholds that are multiples of 1/64 put `d == max_dist` on the boundary.  Asserted on the reference before each device
call: at least half of the 66 page pairs nonzero (54 or 55 are); at least 100 (query, target) pairs exactly on the
threshold where it is a multiple of 1/64 (234 .. 8405; of the SELECTED pairs 2 .. 538, at least 100 in four cases of each
metric); at least 20 selections whose k-th and (k+1)-th nearest are tied (26 .. 2825); at least 10 selections with a
zero-area target inside the top k (48 .. 997).

Further cases on the same table: `valid` set on zero-area rows (they take a max_query slot, count in the valid count of
the other side, and contribute nothing), `valid` cleared on positive-area rows (targets still, queries no more), pages
with fewer valid rows than top_k, one page, a skip matrix, pair-range shards that add up bit for bit, refusals.

Mutants (tests/test_page_pairs_reference_cpu.py asserts that each changes at least 5 page pairs of a grid case): ties
broken by the highest index; `<` for `<=` at the threshold; a zero-area target taking no top-k slot; n_results from the
segment length instead of the valid count; max_query counting invalid rows; a zero-area query taking no max_query slot
(a zero-area query that is merely not skipped cannot be seen: its terms are exact zeros).

MI355X: whole module 3.2 s, slowest test 0.2 s.  The generic-area case, allowed 1e-15, differed by 0 in all three settings.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_pairs_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _emb(t):
    e = _dev(t.x, torch.bfloat16)
    assert np.array_equal(e.float().cpu().numpy(), t.x)  # the bf16 rows are the planted values
    return e


def _run(engine, t, emb, valid, max_query, top_k, threshold, metric, *, normalise=True, skip=None, pair_range=None, area=None):
    S = engine.page_similarity(emb, _dev(t.area if area is None else area), _dev(np.asarray(valid, dtype=np.uint8)), t.offs,
                               None if skip is None else _dev(np.asarray(skip, dtype=np.uint8)), max_query=max_query, top_k=top_k,
                               max_dist=1.0 - threshold, metric=R.METRICS.index(metric), normalise=normalise, pair_range=pair_range)
    torch.cuda.synchronize()
    return S.cpu().numpy()


def _assert_conditions(c, threshold):
    assert 2 * c["nonzero_pairs"] >= c["pairs"], c
    if threshold * 64 == round(threshold * 64):
        assert c["on_threshold"] >= 100, c
    assert c["tied_at_k"] >= 20, c
    assert c["zero_area_in_top_k"] >= 10, c


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("max_query,top_k,threshold", R.GRID)
def test_grid_equals_the_oracle_in_bits(engine, d, metric, max_query, top_k, threshold):
    t = R.table(d)
    valid = t.area > 0
    _assert_conditions(R.conditions(t, valid, max_query, top_k, threshold, metric), threshold)
    want = R.oracle_matrix(t, max_query, top_k, threshold, metric, True)
    want_raw = R.oracle_matrix(t, max_query, top_k, threshold, metric, False)
    assert np.array_equal(want_raw * 2.0 ** 18, np.round(want_raw * 2.0 ** 18))  # exact dyadics: no summation order to match
    emb = _emb(t)
    got = _run(engine, t, emb, valid, max_query, top_k, threshold, metric)
    got_raw = _run(engine, t, emb, valid, max_query, top_k, threshold, metric, normalise=False)
    assert np.array_equal(got_raw, want_raw), np.argwhere(got_raw != want_raw)[:8].tolist()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


def test_selected_pairs_sit_on_the_threshold():
    """the stronger form of the threshold condition: pairs that the top-k SELECTED, so that `<=` is what decides them"""
    t = R.table(64)
    for metric in R.METRICS:
        n = [R.conditions(t, t.area > 0, mq, tk, thr, metric)["selected_on_threshold"] for mq, tk, thr in R.GRID]
        assert sum(v >= 100 for v in n) >= 4, (metric, n)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("max_query,top_k,threshold", [(10, 10, 0.1), (8, 16, 0.5), (2, 64, 0.0)])
def test_valid_zero_area_rows(engine, metric, max_query, top_k, threshold):
    """Every row valid, the zero-area ones too: such a row takes one of the max_query slots and is skipped as a query
    (wrc:203), and counts in the valid count that sets n_results for the other side."""
    t = R.table(64)
    valid = np.ones(t.N, dtype=bool)
    heads = [np.arange(t.offs[p], t.offs[p + 1])[:max_query] for p in range(t.P)]
    assert sum(bool((t.area[h] == 0).any()) for h in heads) >= 5
    want = R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric)
    assert 2 * (np.triu(want, 1) != 0).sum() >= t.P * (t.P - 1) // 2
    assert not np.array_equal(want, R.oracle_matrix(t, max_query, top_k, threshold, metric, False))  # `valid` matters
    got = _run(engine, t, _emb(t), valid, max_query, top_k, threshold, metric, normalise=False)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


@pytest.mark.parametrize("metric", R.METRICS)
def test_valid_cleared_on_positive_area_rows(engine, metric):
    """Such rows are targets still (and may take top-k slots with their area), queries no more, and not counted."""
    t = R.table(64)
    rng = np.random.default_rng(9)
    valid = (t.area > 0) & (rng.random(t.N) < 0.6)
    valid[t.offs[10]: t.offs[11]] = False
    valid[t.offs[10] + 3] = True  # a page of 12 rows with one valid row: n_results = 1 for every query that meets it
    max_query, top_k, threshold = 8, 16, 0.5
    counts = np.array([valid[t.offs[p]: t.offs[p + 1]].sum() for p in range(t.P)])
    assert ((counts > 0) & (counts < top_k)).sum() >= 3, counts  # pages whose valid count is below top_k
    want = R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric)
    assert 2 * (np.triu(want, 1) != 0).sum() >= t.P * (t.P - 1) // 2
    assert not np.array_equal(want, R.oracle_matrix(t, max_query, top_k, threshold, metric, False))
    got = _run(engine, t, _emb(t), valid, max_query, top_k, threshold, metric, normalise=False)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


def test_one_page(engine):
    t = R.table(64)
    one = R.Table()
    one.__dict__.update(t.__dict__)
    one.P, one.N, one.offs = 1, 7, np.array([0, 7], dtype=np.int32)
    one.x, one.area = t.x[:7], t.area[:7]
    emb = _emb(one)
    assert _run(engine, one, emb, one.area > 0, 10, 10, 0.1, "cosine").tolist() == [[1.0]]
    assert _run(engine, one, emb, one.area > 0, 10, 10, 0.1, "cosine", normalise=False).tolist() == [[0.0]]


def test_skip_matrix_and_pair_range_shards(engine):
    t = R.table(64)
    valid = t.area > 0
    max_query, top_k, threshold, metric = 10, 10, 0.5, "cosine"
    emb = _emb(t)
    raw = R.oracle_matrix(t, max_query, top_k, threshold, metric, False)
    skip = np.zeros((t.P, t.P), dtype=np.uint8)
    for i, j in [(0, 2), (0, 11), (3, 7), (1, 10), (4, 5)]:
        assert raw[i, j] > 0
        skip[i, j] = skip[j, i] = 1
    want = R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric, skip=skip)
    assert (want != raw).sum() == 10
    got = _run(engine, t, emb, valid, max_query, top_k, threshold, metric, normalise=False, skip=skip)
    assert np.array_equal(got, want)
    # shards of the upper triangle, bounds that are no multiple of the four pairs a block takes: they add up in bits
    npairs = t.P * (t.P - 1) // 2
    bounds = [0, 1, 7, 22, 23, 49, npairs]
    total = np.zeros_like(raw)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        part = _run(engine, t, emb, valid, max_query, top_k, threshold, metric, pair_range=(lo, hi))
        assert (np.triu(part, 1) != 0).sum() <= hi - lo
        total += part
    assert np.array_equal(total, raw)
    assert np.array_equal(_run(engine, t, emb, valid, max_query, top_k, threshold, metric, pair_range=(5, 5)), np.zeros_like(raw))


def test_generic_areas_within_the_projects_bound(engine):
    """Areas that are no powers of two: the sums now round, in numpy's pairwise order, which the kernel restates.  Bound:
    the project's 1e-15 absolute on the raw matrix (entries are below 0.25 here)."""
    t = R.table(64)
    rng = np.random.default_rng(4)
    area = np.exp(rng.uniform(np.log(1e-2), np.log(20.0), t.N))
    area[t.area == 0] = 0.0
    valid = area > 0
    for max_query, top_k, threshold, metric in [(10, 10, 0.1, "cosine"), (1, 128, 0.5, "cosine"), (16, 8, 0.75, "sqeuclidean")]:
        want = R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric, area=area)
        assert 2 * (np.triu(want, 1) != 0).sum() >= t.P * (t.P - 1) // 2 and want.max() < 0.25
        got = _run(engine, t, _emb(t), valid, max_query, top_k, threshold, metric, normalise=False, area=area)
        diff = np.abs(got - want).max()
        print(f"generic areas {max_query, top_k, threshold, metric}: max |got - want| = {diff:.3e}")
        assert diff <= 1e-15
        assert np.array_equal(got == 0, want == 0)


def test_refusals_leave_the_engine_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError

    t = R.table(64)
    valid = t.area > 0
    emb = _emb(t)
    for kw, metric in [({"max_query": 43, "top_k": 3}, "cosine"), ({"max_query": 129, "top_k": 1}, "cosine"), ({"max_query": 10, "top_k": 0}, "cosine")]:
        assert kw["top_k"] == 0 or kw["max_query"] * kw["top_k"] == 129
        with pytest.raises(MmeError, match="max_query"):
            _run(engine, t, emb, valid, kw["max_query"], kw["top_k"], 0.1, metric)
    with pytest.raises(MmeError, match="metric"):
        engine.page_similarity(emb, _dev(t.area), _dev(valid.astype(np.uint8)), t.offs, None, metric=2)
    got = _run(engine, t, emb, valid, 10, 10, 0.1, "cosine")
    assert np.array_equal(got, R.oracle_matrix(t, 10, 10, 0.1, "cosine", True))
