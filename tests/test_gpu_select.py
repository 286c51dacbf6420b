"""The three launches of K12 (ranked neighbour lists), one at a time through mme_select_apply on planted values:
op 0 topk_rows, op 1 topk_candidates (the candidate-list form of the same selection), op 2 the EPI_TOPK epilogue of the
256 x 256 GEMM.  All comparisons are bit for bit: there is no tolerance anywhere in this file.

Reference.  `select_ref`, numpy, written from the definition in include/mme.h under K12, not from kernel code: for the query
with index self over (value, id) pairs -- (1) order by value descending, id ascending; (2) cut at `fetch`; (3) drop self unless
keep_self; (4) drop id != self with group[id] == group[self]; (5) drop values outside the closed window [min_sim, max_sim];
(6) keep the first top_n; (7) pad with (-1, 0.0f).  Values compare as floats: -0.0 == +0.0 (the id decides), -inf is a value
like any other and enters a list that is not yet full.  NaN values are NOT covered: the contract of K12 is cosines of finite
rows, a NaN never compares greater and the definition gives it no rank, so no table holds one.  One test without a device
runs the whole op-0 table through oracle.compare.neighbour_lists(sim=...) as well and demands equality, which ties this
reference to the one the reference project's own picks pin (tests/test_oracle_pins.py).
Every output (idx_out, sim_out; cand_val, cand_idx, cand_count, overflow) sits between guard rows pre-filled with a sentinel NaN
bit pattern (0x7FA5A5A5) that must be unchanged afterwards, as must every slot the definition leaves unwritten.

(a) op 0 on planted rows (table OP0, built by `op0_cases`; its coverage is asserted by test_tables_cover_what_they_claim).
    Row shapes: strictly ascending (every value inserts at position 0 and the whole list shifts, with the carry from lane 63
    into the high register when fetch > 64), strictly descending (`fetch` appends, then nothing), all equal, a few distinct
    integers at random, tie blocks [3, 5), [6, 13), [254, 258), [510, 514) that cross j % 4 = 3 | 0 and j % 256 = 255 | 0, one
    strict maximum over a constant row at j in {0, 3, 4, 255, 256, N - 1}, seeded normal floats, and rows holding -inf and both
    signed zeros.  Widths N in {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 1023}, each with ld = N rounded up to 4 and with a
    larger pitch; the pad columns [N, ld) hold +inf, so that a read beyond N tops the list and is seen (a NaN there would
    never be inserted and would hide the read).  fetch in {1, 2, 63, 64, 65, 127, 128}, top_n in {1, 10, 64, 65, 128}, including
    top_n > fetch, N < fetch and top_n > 64 with fewer survivors; nrows in {1, 3, 4, 5, 9} (four waves share a workgroup);
    row0 > 0 with a group array longer than row0 + nrows; a group in which the query's own page holds all of the best `fetch`
    values (all -1); keep_self 0 / 1 with and without group; min_sim / max_sim equal to values of the row (both ends
    inclusive); empty windows; cases where `fetch` rows are taken first and fewer than top_n survive although later rows
    would pass the filters; run_if NULL, a device 1, and a device 0 (the outputs keep their sentinel).
(b) op 1 on planted lists (table OP1).  (value, id) sets from the row shapes of (a), written into [nrows, cap] in four orders
    -- id ascending, id descending, two seeded shuffles --, different rows of one launch in different orders, every row in
    every order over the four launches of a case; the result must equal the reference on the SET.  Slots [len, cap) hold
    (+inf, id 0) and must not be read.  len in {0, 1, 3, 4, 5, fetch - 1, fetch, fetch + 1, cap - 1, cap, cap + 7} (the last is
    read as cap), cap in {4, 256, 8192}.  Without a group the ids of every other row lie around 2^30; with one they stay inside
    it; self is present in some lists and absent from others.
(c) op 2 on exact operands (table OP2).  A, W small integers (|a w| <= 9), K in {128, 192, 256}: every partial sum is an
    integer far below 2^24 (asserted: sum |a w| < 2^24), so f32 accumulation is exact in any order and acc is known exactly
    from a float64 matmul.  thr[m * thr_stride] is planted per row from the row's own sorted values, so that values equal to
    the threshold abound and, within one launch, the row counts take each of 0 (+inf), 1, cap - 1, cap, cap + 1 and N (-inf);
    thr_stride 1 and 5 with NaN in the unread slots.  M in {1, 255, 256, 257, 300}, N in {256, 259, 260, 511}, cap in {4, 256},
    and M = 4352, N = 4096, K = 128: 272 tiles for the 256 workgroups of the persistent kernel.  Asserted: cand_count[m] == the
    number of acc[m, n] >= thr[m], n < N, counted past cap; rows with count <= cap hold exactly that set of (n, value) pairs
    in slots [0, count) (compared after sorting by n) and their sentinel behind; rows with count > cap hold cap distinct
    pairs of the set; overflow == 1 iff some count exceeds cap, else still 0, its neighbours untouched; rows >= M untouched.
(d) The chain as mme_neighbours runs it: op 2 then op 1 against gemm_apply(epilogue 4, variant 3) then op 0, bit for bit, and
    both against the reference on the f32 block -- on integer operands, and on seeded random unit bf16 rows with thr = the
    fetch-th best of every 8th column of that block (the sampling rule of mme_neighbours).  No list overflows (asserted).
(e) Sharpness, without a device.  Each plausible bug is a change of the REFERENCE (`mut`), and test_every_mutant_is_caught
    proves that each differs from the true reference on at least one case of the tables: ties broken by descending id; by
    list position (op 1); fetch applied after the filters; window open at the lower / at the upper end; self dropped even
    under keep_self; the group test also applied to self; padding that leaves sim unset; pad columns read; len > cap read
    past cap; the epilogue's >= turned into >; n < N rounded up to 4; the threshold taken from row m + 16; thr_stride ignored;
    the overflow flag raised at count == cap.
(f) Argument validation: each documented precondition returns MME_E_ARG with its message and leaves the sentinel-filled
    outputs untouched.  Only invalid-argument returns are exercised.
"""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

DEV = "cuda"
SENT32 = 0x7FA5A5A5  # an f32 NaN
F32, I32, F64, BF16 = torch.float32, torch.int32, torch.float64, torch.bfloat16
NINF, PINF = float("-inf"), float("inf")


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


class Guard:
    """rows x n 32-bit elements between `guard` rows of sentinel; `fill` (bits) initialises the valid block instead of the sentinel"""

    def __init__(self, dtype, rows, n, guard=3, fill=None):
        self.rows, self.n, self.g = rows, n, guard
        self.raw = torch.full(((rows + 2 * guard) * n,), SENT32, dtype=I32, device=DEV)
        self.view = self.raw.view(dtype).view(rows + 2 * guard, n)[guard : guard + rows]  # what the kernel gets
        if fill is not None:
            self.bits().fill_(fill)

    def bits(self):
        return self.raw.view(self.rows + 2 * self.g, self.n)[self.g : self.g + self.rows]

    def check(self, what):
        b = self.raw.view(self.rows + 2 * self.g, self.n)
        assert bool((b[: self.g] == SENT32).all()) and bool((b[self.g + self.rows :] == SENT32).all()), f"{what}: guard rows overwritten"

    def untouched(self):
        return bool((self.raw == SENT32).all())


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want):
        bad = got != want
        first = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits; first at {list(first)}: "
                             f"got {int(got[first]) & 0xFFFFFFFF:#x} want {int(want[first]) & 0xFFFFFFFF:#x}; rows affected {int(bad.any(-1).sum())}")


# ---------------------------------------------------------------------------------------------------------------------
# the reference of ops 0 and 1, and its mutants


def select_ref(vals, ids, self_id, group, fetch, top_n, keep_self, min_sim, max_sim, mut=""):
    """(value, id) pairs of one query -> (idx int32 [top_n], bits of sim int32 [top_n]); the pairs are given in list order,
    which only the mutant 'tie_position' looks at"""
    vals, ids = np.asarray(vals, np.float32), np.asarray(ids, np.int64)
    if mut == "tie_desc_id":
        order = np.lexsort((-ids, -vals))
    elif mut == "tie_position":
        order = np.argsort(-vals, kind="stable")
    else:
        order = np.lexsort((ids, -vals))  # value descending, id ascending
    lo, hi = np.float32(min_sim), np.float32(max_sim)

    def passes(v, i):
        if i == self_id:
            if not keep_self or mut == "self_always_dropped":
                return False
            if mut == "group_on_self" and group is not None:
                return False
        elif group is not None and group[i] == group[self_id]:
            return False
        return bool((v > lo if mut == "open_lower" else v >= lo) and (v < hi if mut == "open_upper" else v <= hi))

    idx, sim, k = np.full(top_n, -1, np.int32), np.zeros(top_n, np.float32), 0
    for pos, o in enumerate(order):
        if k == top_n:
            break
        if mut == "fetch_after_filters":
            if k == fetch:
                break
        elif pos == fetch:
            break
        if passes(vals[o], int(ids[o])):
            idx[k], sim[k] = ids[o], vals[o]
            k += 1
    bits = sim.view(np.int32).copy()
    if mut == "pad_sim_unset":
        bits[k:] = SENT32
    return idx, bits


# ---------------------------------------------------------------------------------------------------------------------
# (a) the op-0 table

WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 1023)
FETCHES = (1, 2, 63, 64, 65, 127, 128)
TOPNS = (1, 10, 64, 65, 128)
NROWS = (1, 3, 4, 5, 9)
SHAPES = ("asc", "desc", "const", "ints", "blocks", "normal", "special", "max@0", "max@3", "max@4", "max@255", "max@256", "max@last")


def make_row(shape, N, rng):
    """one planted row of N f32 values"""
    j = np.arange(N)
    if shape == "asc":
        v = j.astype(np.float32)
    elif shape == "desc":
        v = -j.astype(np.float32)
    elif shape == "const":
        v = np.full(N, 2.5, np.float32)
    elif shape == "ints":
        v = rng.integers(-2, 3, N).astype(np.float32)
    elif shape == "blocks":
        v = (-1.0 - (j % 7)).astype(np.float32)
        for a, b, x in ((6, 13, 3.0), (510, 514, 3.0), (3, 5, 4.0), (254, 258, 4.0)):
            v[a:b] = x
    elif shape.startswith("max@"):
        v = np.ones(N, np.float32)
        p = N - 1 if shape == "max@last" else min(int(shape[4:]), N - 1)
        v[p] = 2.0
    elif shape in ("normal", "special"):
        v = rng.standard_normal(N).astype(np.float32)
        if shape == "special":
            v[::5] = -np.inf
            v[1::7] = 0.0
            v[2::7] = -0.0
    else:
        raise ValueError(shape)
    return v


def _op0_case(name, N, shapes, seed, *, fetch, top_n, pitch=0, row0=0, group=None, keep_self=0, min_sim=NINF, max_sim=PINF, run_if=None):
    """group: None, or f(length) -> int32 array; the array is max(ld, row0 + nrows) + 3 long (longer than row0 + nrows, and
    long enough for the 'pad columns read' mutant to index it)"""
    rng = np.random.default_rng(seed)
    nrows, ld = len(shapes), -(-N // 4) * 4 + pitch
    rows = np.full((nrows, ld), np.inf, np.float32)
    for r, s in enumerate(shapes):
        rows[r, :N] = make_row(s, N, rng)
    g = None if group is None else np.ascontiguousarray(group(max(ld, row0 + nrows) + 3), dtype=np.int32)
    if callable(min_sim):
        min_sim = min_sim(rows)
    if callable(max_sim):
        max_sim = max_sim(rows)
    return dict(name=name, N=N, ld=ld, rows=rows, shapes=tuple(shapes), row0=row0, group=g, fetch=fetch, top_n=top_n, keep_self=keep_self,
                min_sim=float(np.float32(min_sim)), max_sim=float(np.float32(max_sim)), run_if=run_if)


def _rank(r, k):
    """rows -> the k-th best value (0-based) of row r"""
    return lambda rows: np.sort(rows[r][np.isfinite(rows[r]) | (rows[r] == -np.inf)])[::-1][k]


def _pages(n_pages, seed):
    return lambda length: np.random.default_rng(seed).integers(0, n_pages, length)


@functools.lru_cache(maxsize=None)
def op0_cases():
    cases = []
    # every width, tight and with a larger pitch; nrows, fetch, top_n and the shapes cycle
    for i, N in enumerate(WIDTHS):
        for k, pitch in enumerate((0, 12)):
            n = 2 * i + k
            nrows = NROWS[n % 5]
            shapes = [SHAPES[(3 * n + t) % len(SHAPES)] for t in range(nrows)]
            cases.append(_op0_case(f"w{N}-p{pitch}", N, shapes, 100 + n, fetch=FETCHES[n % 7], top_n=TOPNS[(n + n // 5) % 5], pitch=pitch,
                                   run_if=1 if n % 8 == 3 else None))
    # every fetch over every shape: nine rows and four
    for i, f in enumerate(FETCHES):
        N = (260, 1023, 257)[i % 3]
        cases.append(_op0_case(f"f{f}-shapes9", N, SHAPES[:9], 200 + i, fetch=f, top_n=TOPNS[i % 5]))
        cases.append(_op0_case(f"f{f}-shapes4", N, SHAPES[9:], 220 + i, fetch=f, top_n=TOPNS[(i + 2) % 5], pitch=4 * (i % 2)))
    # row0 > 0, a group array longer than row0 + nrows
    cases.append(_op0_case("row0-group", 260, ["ints"] * 5, 300, fetch=64, top_n=10, row0=100, group=_pages(6, 1), run_if=1))
    # the query's own page holds all of the best `fetch` values: all -1, although every later row would pass (fetch x filters)
    own = lambda length: np.where(np.arange(length) >= 196, 0, 1 + np.arange(length) % 3)
    cases.append(_op0_case("own-page-lo", 260, ["asc"] * 4, 301, fetch=64, top_n=10, row0=200, group=own))
    cases.append(_op0_case("own-page-hi", 260, ["asc"] * 3, 302, fetch=64, top_n=128, row0=200, group=own, keep_self=1))
    # keep_self 0 / 1, with and without group
    for ks in (0, 1):
        for grp in (None, _pages(4, 2)):
            cases.append(_op0_case(f"self{ks}-{'group' if grp else 'nogroup'}", 65, ["ints", "normal", "const"], 310, fetch=64, top_n=64, keep_self=ks, group=grp))
    # windows whose ends are values of the row: both ends inclusive
    cases.append(_op0_case("window-ints", 257, ["ints"] * 4, 320, fetch=128, top_n=128, min_sim=-1.0, max_sim=1.0))
    cases.append(_op0_case("window-ranks", 256, ["normal"] * 4, 321, fetch=64, top_n=10, min_sim=_rank(0, 20), max_sim=_rank(0, 5), keep_self=1))
    cases.append(_op0_case("window-zeros", 260, ["special"] * 3, 322, fetch=128, top_n=65, min_sim=0.0, max_sim=-0.0, keep_self=1))
    # empty windows
    cases.append(_op0_case("window-empty", 64, ["ints"] * 3, 323, fetch=63, top_n=10, min_sim=1.0, max_sim=-1.0))
    cases.append(_op0_case("window-void", 64, ["ints", "normal", "const"], 324, fetch=65, top_n=65, min_sim=2.25, max_sim=2.375))
    # the cut at fetch comes first: ranks 60..62 survive the window, top_n = 10 stays unfilled although later rows would pass
    cases.append(_op0_case("fetch-then-window", 1023, ["normal"] * 5, 325, fetch=63, top_n=10, max_sim=_rank(0, 60), keep_self=1))
    # run_if == 0: nothing is written (low and high register forms)
    cases.append(_op0_case("runif0-lo", 260, ["normal", "ints", "asc"], 330, fetch=64, top_n=10, run_if=0))
    cases.append(_op0_case("runif0-hi", 260, ["normal", "ints", "asc", "desc", "const"], 331, fetch=128, top_n=128, run_if=0))
    return tuple(cases)


def op0_ref(c, mut=""):
    """-> (idx int32 [nrows, top_n], bits of sim int32 [nrows, top_n])"""
    N = c["ld"] if mut == "pad_columns_read" else c["N"]
    out = [select_ref(c["rows"][r, :N], np.arange(N), c["row0"] + r, c["group"], c["fetch"], c["top_n"], c["keep_self"], c["min_sim"], c["max_sim"], mut)
           for r in range(c["rows"].shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def op0_want(i):
    return op0_ref(op0_cases()[i])


# ---------------------------------------------------------------------------------------------------------------------
# (b) the op-1 table

ORDERS = ("id ascending", "id descending", "shuffle A", "shuffle B")
# (cap, fetch, top_n, with group, row0)
OP1 = ((4, 2, 10, False, 0), (4, 64, 1, True, 3), (256, 63, 64, False, 2), (256, 65, 10, True, 0), (256, 128, 128, False, 0),
       (8192, 127, 65, True, 5), (8192, 64, 10, False, 1), (8192, 1, 1, False, 0))
OP1_SHAPES = ("ints", "const", "blocks", "normal", "ints", "special", "asc", "desc", "ints", "max@3", "normal")


def op1_lens(cap, fetch):
    """the row after the cap + 7 row is full, so that the 'len > cap read past cap' mutant meets real values there"""
    return (cap + 7, cap, cap - 1, fetch + 1, fetch, fetch - 1, 5, 4, 3, 1, 0)


@functools.lru_cache(maxsize=None)
def op1_cases():
    cases = []
    for ci, (cap, fetch, top_n, grouped, row0) in enumerate(OP1):
        rng = np.random.default_rng(500 + ci)
        lens = op1_lens(cap, fetch)
        nrows = len(lens)
        G = cap + row0 + nrows + 16
        group = rng.integers(0, 5, G).astype(np.int32) if grouped else None
        rows = []
        for r, ln in enumerate(lens):
            n, self_id = min(ln, cap), row0 + r
            vals = make_row(OP1_SHAPES[r], n, rng) if n else np.zeros(0, np.float32)
            if grouped:  # ids inside the group; self present in the lists of even rows, absent from those of odd rows
                ids = np.sort(rng.choice(G, n, replace=False)).astype(np.int64)
                if n and r % 2 == 0 and self_id not in ids:
                    ids[rng.integers(n)] = self_id
                elif r % 2 == 1 and self_id in ids:
                    ids[ids == self_id] = next(x for x in range(G) if x not in ids)
                ids = np.sort(ids)
            elif r % 2 == 0:  # around 2^30: self absent
                ids = (1 << 30) - n // 2 + np.arange(n, dtype=np.int64)
            else:  # plain column ids: self present where self < n
                ids = np.arange(n, dtype=np.int64)
            assert len(set(ids.tolist())) == n and (n == 0 or (ids.min() >= 0 and ids.max() < 2**31 - 1))
            perms = (np.arange(n), np.arange(n)[::-1], np.random.default_rng(900 + r).permutation(n), np.random.default_rng(950 + r).permutation(n))
            rows.append(dict(len=ln, vals=vals, ids=ids, self_id=self_id, perms=perms))
        cases.append(dict(name=f"cap{cap}-f{fetch}-t{top_n}-{'group' if grouped else 'bigids'}", cap=cap, fetch=fetch, top_n=top_n, row0=row0, group=group,
                          rows=rows, keep_self=ci % 2, min_sim=-1.0 if ci % 3 == 0 else NINF, max_sim=2.5 if ci % 3 == 0 else PINF))
    return tuple(cases)


def op1_lists(c, rot):
    """the [nrows, cap] buffers of launch `rot`: row r is written in order (r + rot) % 4; slots [len, cap) hold (+inf, id 0)"""
    nrows, cap = len(c["rows"]), c["cap"]
    val, idx = np.full((nrows, cap), np.inf, np.float32), np.zeros((nrows, cap), np.int32)
    for r, row in enumerate(c["rows"]):
        p = row["perms"][(r + rot) % 4]
        val[r, : len(p)], idx[r, : len(p)] = row["vals"][p], row["ids"][p]
    return val, idx, np.array([row["len"] for row in c["rows"]], np.int32)


def op1_ref(c, mut="", rot=0):
    val, idx, lens = op1_lists(c, rot)
    out = []
    for r, row in enumerate(c["rows"]):
        n = min(int(lens[r]), c["cap"])
        v, i = val[r, :n], idx[r, :n].astype(np.int64)
        if mut == "len_past_cap":  # reads on into the next row of the buffer
            n = int(lens[r])
            v, i = val.reshape(-1)[r * c["cap"] :][:n], idx.reshape(-1)[r * c["cap"] :][:n].astype(np.int64)
        out.append(select_ref(v, i, row["self_id"], c["group"], c["fetch"], c["top_n"], c["keep_self"], c["min_sim"], c["max_sim"], mut))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def op1_want(i):
    return op1_ref(op1_cases()[i])


# ---------------------------------------------------------------------------------------------------------------------
# (c) the op-2 table.  Operands are made with the CPU generator (the same bits with and without a device); acc, the planted
# thresholds and the expected sets are computed wherever the operands live.

# (M, N, K, cap, thr_stride, overflow planted)
OP2 = ((1, 256, 128, 4, 1, False), (1, 260, 192, 4, 5, True), (255, 259, 192, 4, 5, True), (256, 260, 256, 256, 1, True), (257, 511, 128, 256, 5, True),
       (300, 256, 192, 4, 1, True), (300, 511, 256, 4, 5, True), (257, 259, 128, 256, 1, True), (300, 511, 192, 256, 1, False), (255, 260, 256, 4, 5, False),
       (4352, 4096, 128, 256, 1, True))
OP2_SMALL = OP2[:-1]


def int_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).to(BF16)
    W = torch.randint(-3, 4, (N, K), generator=g).to(BF16)
    return A, W


def exact_acc(A, W):
    """f64 acc, asserted exact under f32 accumulation in any order"""
    assert float((A.double().abs() @ W.double().abs().T).max()) < 2.0**24, "sum |a w| reaches 2^24: accumulation not exact in every order"
    acc = A.double() @ W.double().T
    assert torch.equal(acc.float().double(), acc)
    return acc


def plant_thresholds(acc, cap, overflow, seed):
    """per-row thresholds from the row's own sorted values -> (thr f32 [M], targets: {count: row} of the planted counts).
    A row can take the count c exactly iff its sorted values drop strictly between positions c - 1 and c; rows are searched
    for such drops.  Every other row gets the value at a seeded rank, i.e. a count at least that rank, with ties."""
    M, N = acc.shape
    s = torch.sort(acc, dim=1, descending=True).values
    g = torch.Generator().manual_seed(seed)
    top = min(cap, N) if not overflow else N
    ranks = torch.randint(1, top + 1, (M,), generator=g).to(acc.device)  # 1-based
    thr = s[torch.arange(M, device=acc.device), ranks - 1].clone()
    if not overflow:  # a tie block that reaches past cap would overflow: lower the rank until the count fits
        cnt = (acc >= thr[:, None]).sum(1)
        for m in torch.nonzero(cnt > cap).flatten().tolist():
            strict = torch.nonzero(s[m, :cap] > s[m, cap]).flatten() if cap < N else torch.arange(N)
            thr[m] = s[m, int(strict[-1])] if strict.numel() else PINF
    wanted = [1, cap - 1, cap] + ([cap + 1] if overflow else [])
    targets, used = {}, set()
    if M >= 8:
        for c in (x for x in wanted if 1 <= x < N):
            rows = torch.nonzero(s[:, c - 1] > s[:, c]).flatten().tolist()
            m = next(r for r in rows if r not in used)
            thr[m] = s[m, c - 1]
            targets[c] = m
            used.add(m)
        free = [r for r in range(M) if r not in used]
        targets[0] = free[0]
        thr[free[0]] = PINF
        if overflow:
            targets[N] = free[-1]
            thr[free[-1]] = NINF
    elif overflow:  # M = 1: one count above cap
        thr[0] = s[0, cap]
    else:
        strict = torch.nonzero(s[0, :cap] > s[0, cap]).flatten()
        thr[0] = s[0, int(strict[-1])]
    return thr.float(), targets


def epi_ref(acc, thr_buf, stride, cap, mut=""):
    """the definition of the epilogue: acc f64 [M, N], thr_buf f32 [M * stride] -> (count int64 [M], E bool [M, N'], overflow 0 / 1)"""
    M, N = acc.shape
    m = torch.arange(M, device=acc.device)
    if mut == "thr_row16":
        m = (m + 16) % M
    thr = thr_buf[m if mut == "stride_ignored" else m * stride].double()
    if mut == "n_round4":  # columns up to the next multiple of 4: the tile re-reads the last row of W there
        acc = torch.cat([acc, acc[:, -1:].expand(M, -N % 4)], 1)
    E = acc > thr[:, None] if mut == "gt" else acc >= thr[:, None]
    count = E.sum(1)
    over = int(bool((count >= cap).any() if mut == "overflow_at_cap" else (count > cap).any()))
    return count, E, over


def make_op2_case(i, device):
    M, N, K, cap, stride, overflow = OP2[i]
    A, W = (t.to(device) for t in int_operands(M, N, K, 4000 + i))
    acc = exact_acc(A, W)
    thr, targets = plant_thresholds(acc, cap, overflow, 4100 + i)
    thr_buf = torch.full((M * stride,), float("nan"), dtype=F32, device=device)
    thr_buf[torch.arange(M, device=device) * stride] = thr
    return dict(A=A, W=W, acc=acc, thr_buf=thr_buf, targets=targets, M=M, N=N, K=K, cap=cap, stride=stride, overflow=overflow)


@functools.lru_cache(maxsize=None)
def op2_case(i):
    return make_op2_case(i, "cpu")


# ---------------------------------------------------------------------------------------------------------------------
# tests without a device: the reference against the oracle, the tables' coverage, the mutants


def test_reference_equals_the_oracle_loop_on_the_whole_op0_table():
    from oracle import compare as oc

    for ci, c in enumerate(op0_cases()):
        want_idx, want_bits = op0_want(ci)
        for r in range(c["rows"].shape[0]):
            self_id, row = c["row0"] + r, c["rows"][r, : c["N"]].astype(np.float64)[None]
            if c["N"] == 1:  # the oracle indexes a square block by the query: put the row there
                row = np.repeat(row, self_id + 1, 0)
            idx, sim, _ = oc.neighbour_lists(None, c["group"], top_n=c["top_n"], fetch=c["fetch"], sim=row, rows=range(self_id, self_id + 1),
                                             keep_self=bool(c["keep_self"]), min_sim=c["min_sim"], max_sim=c["max_sim"])
            assert_bits(idx[0].astype(np.int32), want_idx[r], f"oracle vs reference, case {c['name']} row {r}: idx")
            assert_bits(sim[0].astype(np.float32).view(np.int32), want_bits[r], f"oracle vs reference, case {c['name']} row {r}: sim")


def test_tables_cover_what_they_claim():
    c0 = op0_cases()
    assert 24 <= len(c0) <= 60 and all(c["rows"].shape[0] <= 12 and c["N"] <= 1100 for c in c0)
    assert not any(np.isnan(c["rows"]).any() for c in c0)
    assert all(bool((c["rows"][:, c["N"] :] == np.inf).all()) for c in c0)
    for N in WIDTHS:  # tight and with a larger pitch
        assert {c["ld"] - -(-N // 4) * 4 > 0 for c in c0 if c["N"] == N} == {False, True}, N
    assert {c["fetch"] for c in c0} == set(FETCHES) and {c["top_n"] for c in c0} >= set(TOPNS)
    assert {c["rows"].shape[0] for c in c0} >= set(NROWS)
    for f in FETCHES:  # every shape under every fetch, at a width with more than one step of 256 where the shape needs it
        assert {s for c in c0 if c["fetch"] == f and c["N"] >= 257 for s in c["shapes"]} == set(SHAPES), f
    assert any(c["top_n"] > c["fetch"] for c in c0) and any(c["N"] < c["fetch"] for c in c0)
    assert any(c["N"] < c["fetch"] and c["fetch"] > 64 for c in c0) and any(c["N"] < c["fetch"] <= 64 for c in c0)
    short = [ci for ci, c in enumerate(c0) if c["top_n"] > 64 and bool(((op0_want(ci)[0] >= 0).sum(1) < c["top_n"]).any())]
    assert any(bool(((op0_want(ci)[0] >= 0).sum(1) < c0[ci]["top_n"] - 64).any()) for ci in short), "no padding run longer than 64"
    assert any(c["row0"] > 0 and c["group"] is not None and len(c["group"]) > c["row0"] + c["rows"].shape[0] for c in c0)
    assert any(c["group"] is not None and c["N"] > c["fetch"] and bool((op0_want(ci)[0] == -1).all()) for ci, c in enumerate(c0))
    assert {(c["keep_self"], c["group"] is not None) for c in c0} == {(0, False), (0, True), (1, False), (1, True)}
    assert any(c["min_sim"] > c["max_sim"] for c in c0)
    assert {c["run_if"] for c in c0} == {None, 0, 1} and {c["fetch"] > 64 for c in c0 if c["run_if"] == 0} == {False, True}
    for c in c0:  # window ends that are meant to occur in the row do
        if c["name"] in ("window-ints", "window-ranks", "fetch-then-window"):
            assert all(np.isinf(e) or bool((c["rows"][0, : c["N"]] == np.float32(e)).any()) for e in (c["min_sim"], c["max_sim"])), c["name"]
    c1 = op1_cases()
    assert {c["cap"] for c in c1} == {4, 256, 8192} and {c["group"] is not None for c in c1} == {False, True}
    for c in c1:
        assert {r["len"] for r in c["rows"]} == {0, 1, 3, 4, 5, c["fetch"] - 1, c["fetch"], c["fetch"] + 1, c["cap"] - 1, c["cap"], c["cap"] + 7}
        assert any(r["len"] % 4 for r in c["rows"]) and len(c["rows"]) <= 12
        present = {bool((r["ids"] == r["self_id"]).any()) for r in c["rows"] if len(r["ids"])}
        assert present == {False, True} or c["cap"] == 4, c["name"]
        if c["group"] is None:
            assert any(r["ids"].max() >= 2**30 > r["ids"].min() for r in c["rows"] if len(r["ids"]) > 1)
        else:
            assert all(r["ids"].max() < len(c["group"]) for r in c["rows"] if len(r["ids"]))
    assert {c[0] for c in OP2} >= {1, 255, 256, 257, 300, 4352} and {c[1] for c in OP2} >= {256, 259, 260, 511, 4096}
    assert {c[2] for c in OP2} == {128, 192, 256} and {c[3] for c in OP2} == {4, 256} and {c[4] for c in OP2} == {1, 5}
    assert -(-4352 // 256) * -(-4096 // 256) == 272
    for i in range(len(OP2_SMALL)):
        c = op2_case(i)
        count, _, over = epi_ref(c["acc"], c["thr_buf"], c["stride"], c["cap"])
        assert over == int(c["overflow"]), OP2[i]
        if c["M"] >= 8:
            want = {0, 1, c["cap"] - 1, c["cap"]} | ({c["cap"] + 1, c["N"]} if c["overflow"] else set())
            assert want <= set(count.tolist()), (OP2[i], sorted(want - set(count.tolist())))
            assert all(int(count[m]) == k for k, m in c["targets"].items())
        assert bool((c["acc"] == c["thr_buf"][:: c["stride"]].double()[:, None]).any(1).sum() >= min(c["M"], 2)), "no value equal to its threshold"


MUTANTS_SELECT = ("tie_desc_id", "fetch_after_filters", "open_lower", "open_upper", "self_always_dropped", "group_on_self", "pad_sim_unset")
MUTANTS_OP2 = ("gt", "n_round4", "thr_row16", "stride_ignored", "overflow_at_cap")


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_every_mutant_is_caught():
    """each mutant of the module docstring (e) differs from the true reference on at least one case of the tables"""
    c0, c1 = op0_cases(), op1_cases()
    for mut in MUTANTS_SELECT + ("pad_columns_read",):
        assert any(_differs(op0_ref(c, mut), op0_want(ci)) for ci, c in enumerate(c0)), f"op 0: mutant '{mut}' survives the table"
    for mut in MUTANTS_SELECT + ("tie_position", "len_past_cap"):
        assert any(_differs(op1_ref(c, mut, rot), op1_want(ci)) for ci, c in enumerate(c1) for rot in range(4)), f"op 1: mutant '{mut}' survives the table"
    for mut in MUTANTS_OP2:
        hit = False
        for i in range(len(OP2_SMALL)):
            c = op2_case(i)
            count, E, over = epi_ref(c["acc"], c["thr_buf"], c["stride"], c["cap"])
            mc, mE, mo = epi_ref(c["acc"], c["thr_buf"], c["stride"], c["cap"], mut)
            hit = hit or (mo != over if mut == "overflow_at_cap" else not torch.equal(mc, count))
        assert hit, f"op 2: mutant '{mut}' survives the table"


def test_orders_of_one_list_give_one_reference():
    """the reference itself does not look at the list order (only the mutant 'tie_position' does)"""
    for ci, c in enumerate(op1_cases()):
        for rot in range(1, 4):
            assert not _differs(op1_ref(c, "", rot), op1_want(ci))


# ---------------------------------------------------------------------------------------------------------------------
# (a) op 0 on the device


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_op0(eng, c, what):
    nrows, top_n = c["rows"].shape[0], c["top_n"]
    idx, sim = Guard(I32, nrows, top_n), Guard(F32, nrows, top_n)
    flag = None if c["run_if"] is None else torch.tensor([7, c["run_if"], 7], dtype=I32, device=DEV)
    eng.select_apply("topk_rows", qsim=_dev(c["rows"]), ld=c["ld"], N=c["N"], nrows=nrows, row0=c["row0"], group=_dev(c["group"]), fetch=c["fetch"],
                     top_n=top_n, keep_self=c["keep_self"], min_sim=c["min_sim"], max_sim=c["max_sim"], idx_out=idx.view, sim_out=sim.view,
                     run_if=None if flag is None else flag[1:2])
    idx.check(what + " idx_out")
    sim.check(what + " sim_out")
    return idx, sim


@gpu
@pytest.mark.parametrize("ci", range(len(op0_cases())), ids=lambda i: op0_cases()[i]["name"])
def test_topk_rows_on_planted_rows(eng, ci):
    c = op0_cases()[ci]
    what = f"topk_rows {c['name']} (N {c['N']} ld {c['ld']} fetch {c['fetch']} top_n {c['top_n']} rows {c['rows'].shape[0]})"
    idx, sim = run_op0(eng, c, what)
    if c["run_if"] == 0:
        assert idx.untouched() and sim.untouched(), f"{what}: run_if == 0 and the launch wrote"
        return
    want_idx, want_bits = op0_want(ci)
    assert_bits(idx.bits().cpu().numpy(), want_idx, what + ": idx")
    assert_bits(sim.bits().cpu().numpy(), want_bits, what + ": sim")


# ---------------------------------------------------------------------------------------------------------------------
# (b) op 1 on the device


def run_op1(eng, c, val, idx_in, lens, what):
    nrows, top_n = val.shape[0], c["top_n"]
    idx, sim = Guard(I32, nrows, top_n), Guard(F32, nrows, top_n)
    eng.select_apply("topk_candidates", cand_val=val, cand_idx=idx_in, len=lens, cap=c["cap"], nrows=nrows, row0=c["row0"], group=_dev(c["group"]),
                     fetch=c["fetch"], top_n=top_n, keep_self=c["keep_self"], min_sim=c["min_sim"], max_sim=c["max_sim"], idx_out=idx.view, sim_out=sim.view)
    idx.check(what + " idx_out")
    sim.check(what + " sim_out")
    return idx.bits().cpu().numpy(), sim.bits().cpu().numpy()


@gpu
@pytest.mark.parametrize("ci", range(len(op1_cases())), ids=lambda i: op1_cases()[i]["name"])
def test_topk_candidates_do_not_depend_on_list_order(eng, ci):
    c = op1_cases()[ci]
    want_idx, want_bits = op1_want(ci)
    for rot in range(4):
        what = f"topk_candidates {c['name']}, row r in order {ORDERS[rot]} + r"
        val, idx_in, lens = (_dev(a) for a in op1_lists(c, rot))
        got_idx, got_bits = run_op1(eng, c, val, idx_in, lens, what)
        assert_bits(got_idx, want_idx, what + ": idx")
        assert_bits(got_bits, want_bits, what + ": sim")


# ---------------------------------------------------------------------------------------------------------------------
# (c) op 2 on the device


def run_op2(eng, A, W, thr_buf, stride, cap, what):
    """one guarded launch -> (count [M] int64, cand_val Guard, cand_idx Guard, overflow int)"""
    M = A.shape[0]
    cnt = Guard(I32, 1, M, guard=64 // max(M, 1) + 1, fill=0)
    val, idx = Guard(F32, M, cap), Guard(I32, M, cap)
    flag = torch.tensor([SENT32, 0, SENT32], dtype=I32, device=DEV)
    eng.select_apply("gemm_topk", A=A, W=W, thr=thr_buf, thr_stride=stride, cand_count=cnt.view, cand_val=val.view, cand_idx=idx.view, cap=cap,
                     overflow=flag[1:2])
    for g, n in ((cnt, "cand_count"), (val, "cand_val"), (idx, "cand_idx")):
        g.check(f"{what} {n}")
    assert flag[0] == SENT32 and flag[2] == SENT32, f"{what}: the ints beside overflow were written"
    return cnt.bits()[0].long(), val, idx, int(flag[1])


def check_op2(c, count, val, idx, over, what):
    M, N, cap = c["M"], c["N"], c["cap"]
    want_count, E, want_over = epi_ref(c["acc"], c["thr_buf"], c["stride"], cap)
    assert_bits(count.cpu().numpy(), want_count.cpu().numpy(), what + ": cand_count")
    assert over == want_over, f"{what}: overflow = {over}, expected {want_over} (largest count {int(want_count.max())}, cap {cap})"
    k = torch.arange(cap, device=DEV)[None, :]
    filled = k < want_count.clamp(max=cap)[:, None]
    ib, vb = idx.bits(), val.bits()
    assert bool((ib[~filled] == SENT32).all()) and bool((vb[~filled] == SENT32).all()), f"{what}: a slot behind the list was written"
    n = torch.where(filled, ib, torch.zeros_like(ib)).long()
    assert bool(((n >= 0) & (n < N))[filled].all()), f"{what}: a candidate column outside [0, N)"
    m = torch.arange(M, device=DEV)[:, None].expand(M, cap)
    assert bool(E[m, n][filled].all()), f"{what}: a candidate that does not reach its threshold"
    assert torch.equal(vb[filled], c["acc"].float().view(I32)[m, n][filled]), f"{what}: a candidate value is not acc[m, n]"
    seen = torch.zeros((M, N), dtype=I32, device=DEV)
    seen.index_put_((m[filled], n[filled]), torch.ones((), dtype=I32, device=DEV), accumulate=True)
    assert int(seen.max()) <= 1, f"{what}: a candidate was written twice"
    assert torch.equal(seen.sum(1), want_count.clamp(max=cap)), f"{what}: a row does not hold min(count, cap) distinct candidates"
    # rows with count <= cap: exactly the set, compared after sorting by n
    fits = want_count <= cap
    got_sorted = torch.sort(torch.where(filled, n, torch.full_like(n, N)), dim=1).values
    want_sorted = torch.sort(torch.where(E, torch.arange(N, device=DEV)[None, :].expand(M, N), torch.full((M, N), N, device=DEV)), dim=1).values[:, :cap]
    if want_sorted.shape[1] < cap:
        want_sorted = torch.cat([want_sorted, torch.full((M, cap - want_sorted.shape[1]), N, device=DEV)], 1)
    assert_bits(got_sorted[fits].cpu().numpy(), want_sorted[fits].cpu().numpy(), what + ": candidate columns of the rows that fit, sorted")


@gpu
@pytest.mark.parametrize("i", range(len(OP2)), ids=lambda i: "M{}-N{}-K{}-cap{}-stride{}-{}".format(*OP2[i][:5], "overflow" if OP2[i][5] else "fits"))
def test_gemm_topk_epilogue_on_exact_operands(eng, i):
    c = make_op2_case(i, DEV)
    what = f"gemm_topk M {c['M']} N {c['N']} K {c['K']} cap {c['cap']} thr_stride {c['stride']}"
    count, val, idx, over = run_op2(eng, c["A"], c["W"], c["thr_buf"], c["stride"], c["cap"], what)
    check_op2(c, count, val, idx, over, what)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the chain as mme_neighbours runs it


def run_chain(eng, A, W, thr, group, row0, fetch, top_n, keep_self, min_sim, max_sim, cap, what):
    """-> ((idx, sim bits) through op 2 + op 1, (idx, sim bits) through epilogue 4 + op 0, the f32 block as numpy)"""
    M, N = A.shape[0], W.shape[0]
    ld = -(-N // 4) * 4
    q = Guard(F32, M, ld)
    assert eng.gemm_apply(4, A, W, variant=3, outf=q.view, ldf=ld), "the 256 x 256 kernel did not run"
    q.check(what + " f32 block")
    assert bool((q.bits()[:, N:] == SENT32).all())
    sel = dict(nrows=M, row0=row0, group=group, fetch=fetch, top_n=top_n, keep_self=keep_self, min_sim=min_sim, max_sim=max_sim)
    i0, s0 = Guard(I32, M, top_n), Guard(F32, M, top_n)
    eng.select_apply("topk_rows", qsim=q.view, ld=ld, N=N, idx_out=i0.view, sim_out=s0.view, **sel)
    count, val, idx, over = run_op2(eng, A, W, thr, 1, cap, what)
    assert over == 0 and int(count.max()) <= cap, f"{what}: a list overflowed (largest count {int(count.max())}, cap {cap})"
    assert int(count.min()) >= min(fetch, N), f"{what}: a list is shorter than fetch: the threshold is no lower bound"
    # op 1 reads whole rows of cap: the slots behind the lists hold the sentinel NaN and are not read
    i1, s1 = Guard(I32, M, top_n), Guard(F32, M, top_n)
    eng.select_apply("topk_candidates", cand_val=val.view, cand_idx=idx.view, len=count.to(I32), cap=cap, idx_out=i1.view, sim_out=s1.view, **sel)
    for g in (i0, s0, i1, s1):
        g.check(what)
    return (i1.bits().cpu().numpy(), s1.bits().cpu().numpy()), (i0.bits().cpu().numpy(), s0.bits().cpu().numpy()), q.view[:, :N].cpu().numpy()


def chain_ref(block, group, row0, fetch, top_n, keep_self, min_sim, max_sim):
    g = None if group is None else group.cpu().numpy()
    out = [select_ref(block[r], np.arange(block.shape[1]), row0 + r, g, fetch, top_n, keep_self, min_sim, max_sim) for r in range(block.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@gpu
@pytest.mark.parametrize("kind", ["integers", "unit_rows"])
def test_chain_of_candidate_lists_equals_the_block_path(eng, kind):
    M, N, K, cap, row0, top_n = 300, 1023, 128, 256, 200, 10
    if kind == "integers":  # the operands of (c); thr = the row's fetch-th best value
        fetch = 30
        A, W = (t.to(DEV) for t in int_operands(M, N, K, 4900))
        acc = exact_acc(A, W)
        thr = torch.sort(acc, dim=1, descending=True).values[:, fetch - 1].float().contiguous()
        lo, hi = -20.0, float(thr.max()) - 3.0  # integer window ends inside the lists
    else:  # unit bf16 rows against themselves; thr by the sampling rule of mme_neighbours
        fetch = 8
        g = torch.Generator().manual_seed(4901)
        E = torch.randn((N, K), generator=g)
        W = (E / E.norm(dim=1, keepdim=True)).to(BF16).to(DEV)
        A = W[row0 : row0 + M].contiguous()
        blk = Guard(F32, M, 1024)
        assert eng.gemm_apply(4, A, W, variant=3, outf=blk.view, ldf=1024)
        ns = N // 8
        thr = torch.sort(blk.view[:, : 8 * ns : 8], dim=1, descending=True).values[:, fetch - 1].contiguous()
        lo, hi = NINF, 0.999
    group = torch.from_numpy(np.random.default_rng(4902).integers(0, 7, N).astype(np.int32)).to(DEV)
    for keep_self, grp in ((0, group), (1, None)):
        what = f"chain {kind} keep_self {keep_self} group {'yes' if grp is not None else 'no'}"
        lists, block, q = run_chain(eng, A, W, thr, grp, row0, fetch, top_n, keep_self, lo, hi, cap, what)
        if kind == "integers":
            assert np.array_equal(q.astype(np.float64), acc.cpu().numpy()), f"{what}: the f32 block is not the exact product"
        want = chain_ref(q, grp, row0, fetch, top_n, keep_self, lo, hi)
        assert_bits(block[0], want[0], what + ": block path idx vs reference")
        assert_bits(block[1], want[1], what + ": block path sim vs reference")
        assert_bits(lists[0], block[0], what + ": candidate-list path idx vs block path")
        assert_bits(lists[1], block[1], what + ": candidate-list path sim vs block path")


# ---------------------------------------------------------------------------------------------------------------------
# (f) argument validation


@gpu
def test_select_apply_refuses_bad_arguments(eng):
    from multimodal_embeddings_amd._lib import MmeError

    nrows, N, ld, cap, M, K = 4, 20, 24, 8, 4, 128
    q = torch.zeros((nrows + 1, ld), dtype=F32, device=DEV)
    grp = torch.zeros(64, dtype=I32, device=DEV)
    idx, sim = Guard(I32, nrows, 10), Guard(F32, nrows, 10)
    cv_in, ci_in = torch.zeros((nrows + 1, cap), dtype=F32, device=DEV), torch.zeros((nrows + 1, cap), dtype=I32, device=DEV)
    lens = torch.zeros(nrows, dtype=I32, device=DEV)
    A, W = torch.zeros((M + 1, K), dtype=BF16, device=DEV), torch.zeros((N + 1, K), dtype=BF16, device=DEV)
    thr = torch.full((M,), PINF, dtype=F32, device=DEV)
    cnt, cv, ci, flag = Guard(I32, 1, M), Guard(F32, M, cap), Guard(I32, M, cap), Guard(I32, 1, 1)
    ok = {0: dict(qsim=q[:nrows], ld=ld, N=N, nrows=nrows, group=grp, fetch=5, top_n=10, idx_out=idx.view, sim_out=sim.view),
          1: dict(cand_val=cv_in[:nrows], cand_idx=ci_in[:nrows], len=lens, cap=cap, nrows=nrows, group=grp, fetch=5, top_n=10, idx_out=idx.view, sim_out=sim.view),
          2: dict(A=A[:M], W=W[:N], M=M, N=N, K=K, thr=thr, thr_stride=1, cand_count=cnt.view, cand_val=cv.view, cand_idx=ci.view, cap=cap, overflow=flag.view)}

    def call(op, **over):
        kw = dict(ok.get(op, ok[0]))
        kw.update(over)
        return lambda: eng.select_apply(op, **kw)

    bad = [
        (call(3), "op 3 outside 0..2"), (call(-1), "op -1 outside 0..2"),
        (call(0, nrows=-1), "nrows = -1"), (call(1, nrows=-1), "nrows = -1"), (call(0, row0=-2), "row0 = -2"),
        (call(0, fetch=0), "fetch = 0"), (call(0, fetch=129), "fetch = 129"), (call(1, fetch=0), "fetch = 0"), (call(1, fetch=129), "fetch = 129"),
        (call(0, top_n=0), "top_n = 0"), (call(0, top_n=129), "top_n = 129"), (call(1, top_n=0), "top_n = 0"), (call(1, top_n=129), "top_n = 129"),
        (call(0, idx_out=None), "idx_out and sim_out"), (call(0, sim_out=None), "idx_out and sim_out"),
        (call(1, idx_out=None), "idx_out and sim_out"), (call(1, sim_out=None), "idx_out and sim_out"),
        (call(0, qsim=None), "qsim non-null"), (call(0, qsim=q.view(-1)[1 : 1 + nrows * ld]), "qsim non-null and 16-byte aligned"),
        (call(0, ld=22), "ld = 22"), (call(0, ld=16), "ld = 16, N = 20"), (call(0, N=0), "N >= 1 (N = 0)"),
        (call(1, cap=6), "cap = 6"), (call(1, cap=0), "cap = 0"), (call(1, cand_val=None), "cand_val and cand_idx"), (call(1, cand_idx=None), "cand_val and cand_idx"),
        (call(1, len=None), "len non-null"), (call(1, cand_val=cv_in.view(-1)[1 : 1 + nrows * cap]), "16-byte aligned"),
        (call(2, M=-1), "M = -1"), (call(2, N=0), "N = 0"), (call(2, K=64), "K = 64"), (call(2, K=160), "K = 160"), (call(2, cap=0), "cap = 0"),
        (call(2, thr_stride=0), "thr_stride = 0"), (call(2, A=None), "A and W"), (call(2, W=None), "A and W"),
        (call(2, A=A.view(-1)[4 : 4 + M * K].view(M, K)), "A and W non-null and 16-byte aligned"),
        (call(2, W=W.view(-1)[4 : 4 + N * K].view(N, K)), "A and W non-null and 16-byte aligned"),
        (call(2, thr=None), "thr, cand_count"), (call(2, cand_count=None), "thr, cand_count"), (call(2, cand_val=None), "thr, cand_count"),
        (call(2, cand_idx=None), "thr, cand_count"), (call(2, overflow=None), "thr, cand_count"),
    ]
    guards = (idx, sim, cnt, cv, ci, flag)
    for fn, msg in bad:
        with pytest.raises(MmeError) as ei:
            fn()
        assert "(-1)" in str(ei.value) and msg in str(ei.value), f"expected MME_E_ARG with '{msg}', got: {ei.value}"
        assert all(g.untouched() for g in guards), f"a refused call ('{msg}') wrote to its output"
    # the same arguments without the fault are accepted; nrows = 0 and M = 0 launch nothing
    call(0, nrows=0)()
    call(1, nrows=0)()
    call(2, M=0)()
    assert all(g.untouched() for g in guards)
    cnt.bits().fill_(0)
    flag.bits().fill_(0)
    for op in (0, 1, 2):
        call(op)()
    assert int(flag.bits()[0, 0]) == 0 and bool((cnt.bits() == 0).all()) and cv.untouched() and ci.untouched()
