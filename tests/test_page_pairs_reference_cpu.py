"""The planted page-pair inputs (tests/page_pairs_reference.py) without a GPU: that the expected output is exact, that no
case is vacuous, and that each named mutant is visible -- known to hold before anything reaches a GPU.

Reference: oracle.compare.compute_image_similarity_matrix on float64 host cosines.  `page_matrix`, the switchable
restatement the mutants are written in, must equal it in bits on every grid case (both are exact: every term is a
multiple of 2^-18 and every sum stays below 2^7).  Each mutant must change at least 5 page pairs of some grid case;
"a zero-area query takes no max_query slot" is evaluated with every row valid, the only setting in which a zero-area
row can be a query at all.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_pairs_reference as R  # noqa: E402


@pytest.mark.parametrize("metric", R.METRICS)
def test_restatement_equals_the_oracle_and_no_case_is_vacuous(metric):
    t = R.table(64)
    valid = t.area > 0
    for max_query, top_k, threshold in R.GRID:
        assert max_query * top_k <= 128
        for normalise in (False, True):
            want = R.oracle_matrix(t, max_query, top_k, threshold, metric, normalise)
            assert np.array_equal(R.page_matrix(t, valid, max_query, top_k, threshold, metric, normalise), want)
        want_raw = R.oracle_matrix(t, max_query, top_k, threshold, metric, False)
        assert np.array_equal(R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric), want_raw)
        assert np.array_equal(want_raw * 2.0 ** 18, np.round(want_raw * 2.0 ** 18)) and want_raw.max() < 128
        c = R.conditions(t, valid, max_query, top_k, threshold, metric)
        print(metric, (max_query, top_k, threshold), c)
        assert 2 * c["nonzero_pairs"] >= c["pairs"], c
        if threshold * 64 == round(threshold * 64):
            assert c["on_threshold"] >= 100, c
        assert c["tied_at_k"] >= 20 and c["zero_area_in_top_k"] >= 10, c
    assert any(mq * tk == 128 for mq, tk, _ in R.GRID)


def test_the_wider_table_holds_the_same_cosines():
    t64, t128 = R.table(64), R.table(128)
    assert t128.x.shape == (t64.N, 128) and np.array_equal(t128.C, t64.C)
    assert set(np.unique(np.abs(t128.x)).tolist()) == {0.0, 0.125}
    # exact duplicates, inside a page and across pages
    assert np.array_equal(t64.x[20:29], np.tile(t64.x[3], (9, 1))) and np.array_equal(t64.x[t64.offs[9]], t64.x[t64.offs[10]])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_change_page_pairs(mutant):
    t = R.table(64)
    valid = np.ones(t.N, dtype=bool) if mutant == "zero_area_query_takes_no_slot" else t.area > 0
    best = 0
    for metric in R.METRICS:
        for max_query, top_k, threshold in R.GRID:
            true = R.page_matrix(t, valid, max_query, top_k, threshold, metric, False)
            if mutant == "zero_area_query_takes_no_slot":
                assert np.array_equal(true, R.oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric))
            changed = int((np.triu(R.page_matrix(t, valid, max_query, top_k, threshold, metric, False, mutant), 1) != np.triu(true, 1)).sum())
            best = max(best, changed)
    print(f"{mutant}: changes up to {best} of 66 page pairs")
    assert best >= 5
