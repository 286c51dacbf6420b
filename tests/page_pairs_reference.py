"""Planted inputs of the page-pair reduction (K10) whose expected output is exact, and a switchable restatement of its
selection rule for the mutants.

The reference of the GPU tests is oracle.compare (`compute_image_similarity_matrix`, `pair_terms`) fed with float64 dot
products of the bf16 rows computed on the host.  `page_matrix` below restates the same rule with one numpy sort per
page pair and takes a `mutant` name; without one it must equal the oracle bit for bit (asserted where it is used).

Why the comparison can be exact.  Rows have entries in {0, +-1/8}: a dot product of d <= 128 of them is a multiple of
1/64 of magnitude <= 2, with sum |a b| <= 2 < 2^24 / 64 (asserted), so it is exact in f32 in any accumulation order and
the device's cosines ARE the float64 ones.  `area_percentage` is 100 / 2^k or 0, so area / 100 = 2^-k exactly, a term
(1 - d) * area_i * area_j is a multiple of 2^-18 below 2, and a sum of at most 128 terms needs 26 bits: exact in f64 in
any order.  Normalisation is one IEEE division per entry by the same maximum.
"""
import functools

import numpy as np

COUNTS = (300, 7, 256, 257, 64, 65, 1, 130, 0, 40, 12, 300)  # rows per page: both selection paths, every register's edge
AREAS = (0.0, 100.0, 50.0, 25.0, 12.5, 6.25, 3.125, 1.5625)
# (max_query, top_k, threshold)
GRID = ((10, 10, 0.1), (16, 8, 0.75), (8, 16, 0.5), (1, 128, 0.5), (128, 1, 0.25), (3, 5, 0.0), (10, 10, 0.5))
GRID = GRID + ((2, 64, 0.0), (4, 32, 0.25))  # top_k above the valid count of six pages, at thresholds most rows pass
METRICS = ("cosine", "sqeuclidean")
MUTANTS = ("highest_index_wins", "strict_threshold", "zero_area_target_takes_no_slot", "n_results_from_segment_length",
           "max_query_counts_invalid_rows", "zero_area_query_takes_no_slot")


class Table:
    """x [N, d] float32 holding the bf16-exact rows, C [N, N] float64 dot products, area [N], page_of [N], offs [P + 1]"""


@functools.lru_cache(maxsize=None)
def table(d=64, seed=5):
    """The planted table.  d = 128 is the d = 64 table with its columns scattered over 128 (the rest 0), so rows keep their
    unit scale and every figure of the 64-column table holds; what changes is the K extent of the cosine GEMM."""
    if d != 64:
        t64 = table(64, seed)
        t = Table()
        t.__dict__.update(t64.__dict__)
        x = np.zeros((t64.N, d), dtype=np.float32)
        x[:, np.sort(np.random.default_rng(seed + 1).permutation(d)[:64])] = t64.x
        t.d, t.x = d, x
        assert np.array_equal(x.astype(np.float64) @ x.astype(np.float64).T, t64.C)
        return t
    rng = np.random.default_rng(seed)
    N, P = sum(COUNTS), len(COUNTS)
    # four centre rows at planted mutual cosines: c1, c2, c3 are c0 with d/8, d/4, d/2 entries flipped (3/4, 1/2, 0)
    c0 = rng.choice([-1.0, 1.0], d)
    centres = np.tile(c0, (4, 1))
    perm = rng.permutation(d)
    centres[1, perm[: d // 8]] *= -1
    centres[2, perm[d // 8: d // 8 + d // 4]] *= -1
    centres[3, perm[d // 2:]] *= -1
    # a page's rows mostly share one centre, so that the nearest rows of another page sit AT a planted cosine
    page_of = np.repeat(np.arange(P), COUNTS)
    which = np.where(rng.random(N) < 0.7, page_of % 4, rng.choice(4, N, p=[0.4, 0.3, 0.2, 0.1]))
    x = centres[which] / 8.0
    # entries changed per row: none or a few (zeroed or flipped), or d/16 .. d/2 zeroed -- against an unchanged row of
    # the same centre that is a cosine of 1 - z/d, i.e. 7/8, 3/4, 5/8, 1/2: the thresholds of the sqeuclidean metric
    planted = [0, 0, 0, 1, 2, 3, d // 16, d // 8, 3 * d // 16, d // 4, 3 * d // 8, d // 2]
    nchg = rng.choice(planted, N)
    for r in range(N):
        idx = rng.choice(d, nchg[r], replace=False)
        flip = (rng.random(nchg[r]) < 0.25) & (nchg[r] <= 3)
        x[r, idx[flip]] *= -1
        x[r, idx[~flip]] = 0.0
    offs = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    # runs of exact duplicates: inside a long page, inside a short one, and of a row of another page
    for p in range(P):  # every page opens with unchanged copies of centre 0: a single query still meets most pages
        x[offs[p]: min(offs[p] + 2, offs[p + 1])] = centres[0] / 8.0
    x[20:29] = x[3]
    x[310:330] = x[2]
    x[offs[3] + 250: offs[3] + 257] = x[offs[2] + 1]
    x[offs[7] + 60: offs[7] + 72] = x[offs[4]]
    x[offs[11] + 100: offs[11] + 140] = x[offs[9] + 5]
    x[offs[9]: offs[9] + 4] = x[offs[10]]
    area = rng.choice(AREAS, N, p=[0.12, 0.05, 0.1, 0.15, 0.2, 0.18, 0.1, 0.1])
    t = Table()
    t.d, t.N, t.P = d, N, P
    t.x = x.astype(np.float32)
    t.C = x @ x.T  # float64, exact (multiples of 1/64)
    assert np.array_equal(t.C * 64, np.round(t.C * 64))
    assert (np.abs(x) @ np.abs(x).T).max() < 2 ** 24 / 64  # f32 accumulation of the products is exact in any order
    t.area = area
    t.page_of = np.repeat(np.arange(P), COUNTS)
    t.offs = offs
    t.names = [f"{p:03d} planted page.png" for p in range(P)]
    return t


def distance(c, metric):
    return 1.0 - c if metric == "cosine" else 2.0 - 2.0 * c


def selections(t, valid, max_query, top_k, threshold, metric, mutant=None):
    """Yields (i, j, area_i [q], d_sel [q, n], area_sel [q, n], d_next [q] or None, d [q, L]) for every page pair i < j that
    the rule evaluates: the selected distances in selection order, the distance of the first row NOT selected, and all."""
    valid = np.asarray(valid, dtype=bool)
    rows = [np.arange(t.offs[p], t.offs[p + 1]) for p in range(t.P)]
    regions = [r[valid[r]] for r in rows]
    for i in range(t.P):
        for j in range(i + 1, t.P):
            if len(regions[i]) == 0 or len(regions[j]) == 0:
                continue
            n = min(top_k, len(rows[j]) if mutant == "n_results_from_segment_length" else len(regions[j]))
            if mutant == "max_query_counts_invalid_rows":
                q = rows[i][:max_query]
                q = q[valid[q]]
            elif mutant == "zero_area_query_takes_no_slot":
                q = regions[i][t.area[regions[i]] > 0][:max_query]
            else:
                q = regions[i][:max_query]
            q = q[t.area[q] > 0]  # a zero-area query contributes nothing (its terms would be exact zeros)
            if len(q) == 0:
                continue
            tgt = rows[j]
            if mutant == "zero_area_target_takes_no_slot":
                tgt = tgt[t.area[tgt] > 0]
            d = distance(t.C[np.ix_(q, tgt)], metric)
            if mutant == "highest_index_wins":
                order = d.shape[1] - 1 - np.argsort(d[:, ::-1], axis=1, kind="stable")
            else:
                order = np.argsort(d, axis=1, kind="stable")
            sel = order[:, :n]
            d_sel = np.take_along_axis(d, sel, axis=1)
            d_next = np.take_along_axis(d, order[:, n: n + 1], axis=1)[:, 0] if d.shape[1] > n else None
            yield i, j, t.area[q] / 100.0, d_sel, t.area[tgt][sel] / 100.0, d_next, d


def page_matrix(t, valid, max_query, top_k, threshold, metric, normalise, mutant=None, skip=None):
    max_dist = 1.0 - threshold
    S = np.zeros((t.P, t.P))
    for i, j, ai, d_sel, aj, _, _ in selections(t, valid, max_query, top_k, threshold, metric, mutant):
        if skip is not None and skip[i, j]:
            continue
        keep = ((d_sel < max_dist) if mutant == "strict_threshold" else (d_sel <= max_dist)) & (aj > 0)
        terms = ((1.0 - d_sel) * ai[:, None] * aj)[keep]
        if len(terms):
            S[i, j] = S[j, i] = np.sum(terms)
    if normalise:
        mx = np.max(S - np.diag(np.diag(S)))
        if mx > 0:
            off = ~np.eye(t.P, dtype=bool)
            S[off] = S[off] / mx
        np.fill_diagonal(S, 1.0)
    return S


def conditions(t, valid, max_query, top_k, threshold, metric):
    """The figures a case must reach to test anything: nonzero page pairs, selected (query, target) pairs exactly on the
    threshold, selections whose k-th and (k+1)-th nearest are tied, selections with a zero-area target inside the top k."""
    max_dist = 1.0 - threshold
    on_threshold = selected_on_threshold = tied = zero_area = 0
    for _, _, _, d_sel, aj, d_next, d_all in selections(t, valid, max_query, top_k, threshold, metric):
        on_threshold += int((d_all == max_dist).sum())
        selected_on_threshold += int((d_sel == max_dist).sum())
        if d_next is not None and d_sel.shape[1]:
            tied += int((d_sel[:, -1] == d_next).sum())
        zero_area += int((aj == 0).any(axis=1).sum())
    S = page_matrix(t, valid, max_query, top_k, threshold, metric, False)
    return {"nonzero_pairs": int((np.triu(S, 1) != 0).sum()), "pairs": t.P * (t.P - 1) // 2, "on_threshold": on_threshold,
            "selected_on_threshold": selected_on_threshold, "tied_at_k": tied,
            "zero_area_in_top_k": zero_area}


def oracle_matrix(t, max_query, top_k, threshold, metric, normalise):
    """oracle.compare on the host's float64 cosines, with valid = (area > 0) as the oracle defines it"""
    from oracle import compare as ocmp

    S, _ = ocmp.compute_image_similarity_matrix(None, t.area, t.page_of, t.names, None, metric=metric, effective_threshold=threshold,
                                                skip_same_prefix=False, max_query_regions=max_query, top_k=top_k, normalise=normalise, sim=t.C)
    return S


def oracle_matrix_valid(t, valid, max_query, top_k, threshold, metric, area=None, skip=None):
    """Raw matrix for an arbitrary `valid`: oracle.compare.pair_terms per pair, regions_i and the valid count of j taken
    from `valid` (a valid zero-area row counts; pair_terms skips it as a query after it took its max_query slot)."""
    from oracle import compare as ocmp

    valid = np.asarray(valid, dtype=bool)
    area = t.area if area is None else area
    rows = [np.arange(t.offs[p], t.offs[p + 1]) for p in range(t.P)]
    regions = [r[valid[r]] for r in rows]
    S = np.zeros((t.P, t.P))
    for i in range(t.P):
        for j in range(i + 1, t.P):
            if len(regions[i]) == 0 or len(regions[j]) == 0 or (skip is not None and skip[i, j]):
                continue
            w = ocmp.pair_terms(None, area, regions[i], rows[j], len(regions[j]), metric=metric, effective_threshold=threshold,
                                max_query_regions=max_query, top_k=top_k, sim=t.C)
            if w:
                S[i, j] = S[j, i] = np.sum(w)
    return S
