"""K15 spherical k-means on the GPU (include/mme.h, mme_kmeans / mme_kmeans_apply): every kernel alone on planted or exact
inputs, the assignment against float64 within K14's bound, whole runs against the float64 restatement
(tests/kmeans_reference.py) on fixtures whose margin is asserted first, the refusals, and the Python layer."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = [64, 384, 512, 768, 1024]
GUARD = 64  # sentinel elements in front of and behind every output


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    return Engine(0)


class Guarded:
    """an output tensor between two runs of sentinels"""

    PATTERN = {torch.int32: -123456789, torch.float32: -7.5e30, torch.float64: -7.5e300, torch.int64: -1234567890123, torch.int16: 0x1234}

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.fill = self.PATTERN[dtype] if fill is None else fill
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD : GUARD + n].view(*shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[-GUARD:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _bf16(bits):
    """uint16 numpy -> bfloat16 CUDA tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _unit_bits(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return R.f64_to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


# ---- ARGMAX on planted blocks ---------------------------------------------------------------------------------------------

def _order_key(v):
    """the total order of the argmax as int64 keys: NaN lowest, then -inf .. -0.0 < +0.0 .. +inf"""
    u = v.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)
    return np.where(np.isnan(v), -1, key)


def _planted_block(rows, k, seed):
    """block [rows, ld] with ld > k and large values behind column k, and what each row was planted for"""
    rng = np.random.default_rng(seed)
    ld = (k + 3) // 4 * 4 + 4
    blk = rng.uniform(-1, 1, size=(rows, ld)).astype(np.float32)
    blk[:, k:] = 9e9  # not valid columns: must never win
    want = np.full(rows, -1)
    for r in range(rows):
        p = r % 8
        if p == 0:
            blk[r, 0], want[r] = 2.0, 0  # the maximum in the first column
        elif p == 1:
            blk[r, k - 1], want[r] = 2.0, k - 1  # and in the last
        elif p == 2:
            lo = k // 3
            blk[r, lo] = blk[r, k - 1] = np.float32(1.7)  # bit-equal maxima far apart: the lowest column
            want[r] = lo
        elif p == 3:
            blk[r, :k] = -0.0
            blk[r, k - 1] = 0.0  # +0.0 is above -0.0 (for k = 1 it is the only value)
            want[r] = k - 1
        elif p == 4:
            blk[r, 0] = np.nan  # a NaN beside numbers loses; alone (k = 1) it is all there is
            if k > 2:
                blk[r, k // 2] = np.nan
            want[r] = -1 if k > 1 else 0
        elif p == 5:
            blk[r, :k] = np.nan  # label 0, sim NaN
            want[r] = 0
        elif p == 6:
            blk[r, :k] = -np.inf
            blk[r, k - 1] = np.float32(-3e38)  # above -inf
            want[r] = k - 1
    return blk, ld, want


@pytest.mark.parametrize("rows", [1, 63, 257])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 257, 1000])
def test_argmax_rows_on_planted_blocks(engine, rows, k):
    blk, ld, want = _planted_block(rows, k, seed=rows * 1009 + k)
    exp = np.argmax(_order_key(blk[:, :k]), axis=1).astype(np.int32)  # the first of equal keys
    planted = want >= 0
    assert np.array_equal(exp[planted], want[planted])
    exp_sim = blk[np.arange(rows), exp]
    prev = exp.copy()
    prev[1::2] = (exp[1::2] + 1) % max(k, 2)  # every odd row held another label before
    n_moved = int((prev != exp).sum())
    assert n_moved == rows // 2
    q = torch.from_numpy(blk).cuda()
    labels, sim = Guarded((rows,), torch.int32), Guarded((rows,), torch.float32)
    moved = torch.tensor([1000], dtype=torch.int64, device="cuda")
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    labels.t.copy_(torch.from_numpy(prev))
    before = labels.buf.clone()
    engine.kmeans_apply("argmax", qsim=q, k=k, labels=labels.t, sim=sim.t, moved=moved, run_if=gate)  # run_if = 0 writes nothing
    assert torch.equal(labels.buf, before) and sim.untouched() and int(moved.item()) == 1000
    gate.fill_(1)
    for run in range(2):  # the second run starts from the first one's labels: nothing moves
        engine.kmeans_apply("argmax", qsim=q, ld=ld, k=k, labels=labels.t, sim=sim.t, moved=moved, run_if=gate if run == 0 else None)
        assert np.array_equal(labels.t.cpu().numpy(), exp)
        assert np.array_equal(sim.t.cpu().numpy().view(np.uint32), exp_sim.view(np.uint32))  # bit for bit, NaN and zeros included
        assert int(moved.item()) == 1000 + n_moved
        assert labels.intact() and sim.intact()


# ---- ASSIGN against float64 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_assign_against_float64(engine, d):
    delta = R.delta(d)
    for N in (1, 255, 300):
        xb = _unit_bits(N, d, seed=d + N)
        x64 = R.bf16_to_f64(xb)
        x = _bf16(xb)
        for k in (1, 7, 65, 257):
            cb = _unit_bits(k, d, seed=7 * d + k)
            if k >= 7:
                cb[3] = cb[1]  # two equal centroids: equal scores, the lower one wins
                cb[k - 1] = xb[N - 1]  # the last row's own vector as the last centroid
            S = x64 @ R.bf16_to_f64(cb).T
            cen = _bf16(cb)
            first = None
            for chunk_rows in (0, 64, 100):
                labels, sim = Guarded((N,), torch.int32), Guarded((N,), torch.float32)
                labels.t.fill_(-1)
                moved = torch.zeros(1, dtype=torch.int64, device="cuda")
                engine.kmeans_apply("assign", emb=x, centroids=cen, chunk_rows=chunk_rows, labels=labels.t, sim=sim.t, moved=moved)
                lab, s = labels.t.cpu().numpy(), sim.t.cpu().numpy()
                assert labels.intact() and sim.intact() and int(moved.item()) == N, (N, k, chunk_rows)
                assert lab.min() >= 0 and lab.max() < k
                got = S[np.arange(N), lab]
                worst = float((S.max(axis=1) - got).max())
                err = float(np.abs(s.astype(np.float64) - got).max())
                assert worst <= 2 * delta and err <= delta, (N, k, chunk_rows, worst / delta, err / delta)
                if k >= 7:
                    assert not (lab == 3).any() and lab[N - 1] == k - 1
                if first is None:
                    first = (lab, s)
                    # a second pass over its own labels moves nothing, through a gate that is open
                    gate = torch.ones(1, dtype=torch.int32, device="cuda")
                    engine.kmeans_apply("assign", emb=x, centroids=cen, labels=labels.t, sim=sim.t, moved=moved, run_if=gate)
                    assert int(moved.item()) == N and np.array_equal(labels.t.cpu().numpy(), lab)
                    gate.zero_()
                    labels.t.fill_(-5)
                    engine.kmeans_apply("assign", emb=x, centroids=cen, labels=labels.t, sim=sim.t, moved=moved, run_if=gate)
                    assert int(moved.item()) == N and bool((labels.t == -5).all()) and np.array_equal(sim.t.cpu().numpy(), s)
                else:  # the chunk edges change no bit
                    assert np.array_equal(lab, first[0]) and np.array_equal(s.view(np.uint32), first[1].view(np.uint32)), (N, k, chunk_rows)


# ---- UPDATE on exactly summable rows ----------------------------------------------------------------------------------------

def _exact_bits(n, d, seed):
    """bf16 rows whose nonzero values are +-2^e (1 + m / 128), -8 <= e <= -2: multiples of 2^-15 below 1/2, so that float64
    adds any number of them (far below 2^38) exactly, in any order"""
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, 2, (n, d)) << 15) | (rng.integers(127 - 8, 127 - 1, (n, d)) << 7) | rng.integers(0, 128, (n, d))
    bits[rng.random((n, d)) < 0.1] = 0
    return bits.astype(np.uint16)


def _update_labels(n, k, kind, seed):
    if kind == "one" or k == 1:
        lab = np.zeros(n, dtype=np.int32) + (k - 1 if kind == "one" else 0)  # one cluster holds every row
    else:
        rng = np.random.default_rng(seed)
        lab = rng.integers(0, k, n).astype(np.int32)
        lab[lab == 2] = 0  # cluster 2 is empty
        lab[lab == k - 1] = 1
        lab[n // 2] = k - 1  # the last cluster has exactly one row
    return lab


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("k", [1, 7, 65])
def test_update_is_exact_and_reproducible(engine, d, k):
    n = 300 if d > 64 else 1000  # two chunks of rows; four at d = 64
    xb = _exact_bits(n, d, seed=d * 3 + k)
    x64 = R.bf16_to_f64(xb)
    nz = np.abs(x64[x64 != 0])
    assert nz.min() >= 2.0 ** -20 and nz.max() < 1  # the sums below are exact and independent of the order
    x = _bf16(xb)
    old = np.full((k, d), 0x3C12, dtype=np.uint16)
    for kind in ("mixed", "one"):
        lab = _update_labels(n, k, kind, seed=k)
        if kind == "mixed" and k > 1:
            lab[5], lab[n - 1] = -1, k  # rows that belong to no cluster
        inside = (lab >= 0) & (lab < k)
        want_counts = np.bincount(lab[inside], minlength=k).astype(np.int32)
        want_sums = np.zeros((k, d))
        np.add.at(want_sums, lab[inside], x64[inside])
        ref_sums, ref_counts, ref_cen = R.update(x64, lab, old)
        assert np.array_equal(ref_sums, want_sums) and np.array_equal(ref_counts, want_counts)  # exact either way
        if kind == "mixed" and k > 1:
            assert want_counts[2] == 0 and want_counts[k - 1] == 1 and np.array_equal(ref_cen[2], old[2])
        else:
            assert want_counts.max() == n
        labels = torch.from_numpy(lab).cuda()
        runs = []
        for run in range(2):
            sums, counts, cen = Guarded((k, d), torch.float64), Guarded((k,), torch.int32), Guarded((k, d), torch.int16)
            if run == 0:  # a closed gate writes nothing
                gate = torch.zeros(1, dtype=torch.int32, device="cuda")
                engine.kmeans_apply("update", emb=x, labels=labels, centroids=cen.t.view(torch.bfloat16), sums=sums.t, counts=counts.t, run_if=gate)
                assert sums.untouched() and counts.untouched() and cen.untouched()
            cen.t.copy_(torch.from_numpy(old.view(np.int16)))
            engine.kmeans_apply("update", emb=x, labels=labels, centroids=cen.t.view(torch.bfloat16), sums=sums.t, counts=counts.t)
            assert sums.intact() and counts.intact() and cen.intact()
            got = (sums.t.cpu().numpy(), counts.t.cpu().numpy(), _bits(cen.t))
            assert np.array_equal(got[1], want_counts)
            assert np.array_equal(got[0].view(np.uint64), want_sums.view(np.uint64)) or np.array_equal(got[0], want_sums)  # -0.0 never arises
            assert np.array_equal(got[2], ref_cen), np.argwhere(got[2] != ref_cen)[:5]
            runs.append(got)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*runs))
        assert torch.equal(labels, torch.from_numpy(lab).cuda())


# ---- whole runs against the restatement -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(name, max_iter):
    x, rows = R.load_case(name)
    return R.run(x, x[rows], max_iter)


def _run_raw(engine, xb, k, rows, max_iter, start_bits=None):
    """mme_kmeans on guarded buffers; -> dict of numpy outputs (sentinels checked)"""
    from multimodal_embeddings_amd._lib import _KmeansState

    N, d = xb.shape
    x = _bf16(xb)
    out = {"centroids": Guarded((k, d), torch.int16), "sums": Guarded((k, d), torch.float64), "counts": Guarded((k,), torch.int32),
           "labels": Guarded((N,), torch.int32), "sim": Guarded((N,), torch.float32), "info": Guarded((4,), torch.int64),
           "objective": Guarded((1,), torch.float64)}
    if start_bits is not None:
        out["centroids"].t.copy_(torch.from_numpy(np.ascontiguousarray(start_bits).view(np.int16)))
    st = _KmeansState()
    for f, g in out.items():
        setattr(st, f, g.t.data_ptr())
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    rc = engine.lib.mme_kmeans(engine.h, x.data_ptr(), N, d, k, None if r is None else r.ctypes.data, max_iter, C.byref(st), engine._stream())
    assert rc == 0, engine.lib.mme_last_error(engine.h).decode()
    torch.cuda.synchronize()
    assert all(g.intact() for g in out.values())
    res = {f: g.t.cpu().numpy() for f, g in out.items()}
    res["centroids"] = res["centroids"].view(np.uint16)
    res["untouched"] = {f: g.untouched() for f, g in out.items()}
    return res


def _same_run(got, ref, d, *, updated=True):
    assert np.array_equal(got["labels"], ref["labels"]), np.argwhere(got["labels"] != ref["labels"])[:5].ravel()
    assert np.array_equal(got["centroids"], ref["centroids"])
    assert got["info"].tolist() == [ref["iterations"], ref["moved"], int(ref["converged"]), ref["empty"]]
    if updated:
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["sums"], ref["sums"])  # the same adds in the same order
    assert float(np.abs(got["sim"].astype(np.float64) - ref["sim"]).max()) <= R.delta(d)
    assert abs(got["objective"][0] - got["sim"].astype(np.float64).sum()) <= 1e-12 * len(got["sim"])


def _describes(got, xb, d):
    """the labels belong to the returned centroids: each within 2 delta of its row's best float64 score"""
    S = R.bf16_to_f64(xb) @ R.bf16_to_f64(got["centroids"]).T
    assert float((S.max(axis=1) - S[np.arange(len(S)), got["labels"]]).max()) <= 2 * R.delta(d)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_whole_run_equals_the_restatement(engine, name):
    n, d, kt, k, noise = R.CASES[name]
    xb, rows = R.load_case(name)
    ref = _reference(name, 50)
    # the condition under which only the GEMM's rounding separates the two runs, and it cannot decide a label
    assert ref["gap"] > 4 * R.delta(d) and ref["converged"] and ref["iterations"] >= 2, (ref["gap"] / R.delta(d), ref["iterations"])
    got = _run_raw(engine, xb, k, rows, 50)
    _same_run(got, ref, d)
    _describes(got, xb, d)
    # the start given as centroids is the same run
    again = _run_raw(engine, xb, k, None, 50, start_bits=xb[rows])
    assert all(np.array_equal(got[f].view(np.uint8), again[f].view(np.uint8)) for f in ("labels", "sim", "centroids", "counts", "sums", "info", "objective"))


@pytest.mark.parametrize("name", ["d64", "d128", "d384"])
def test_runs_cut_short_are_not_converged_and_stay_consistent(engine, name):
    n, d, kt, k, noise = R.CASES[name]
    xb, rows = R.load_case(name)
    full = _reference(name, 50)
    assert full["gap"] > 4 * R.delta(d)
    for max_iter in (0, 1, full["iterations"] - 1):
        ref = _reference(name, max_iter)
        got = _run_raw(engine, xb, k, rows, max_iter)
        _same_run(got, ref, d, updated=max_iter > 0)
        assert got["info"][0] == max_iter and got["info"][2] == 0 and not ref["converged"]
        _describes(got, xb, d)
        if max_iter == 0:  # "assign rows to given centroids": the centroids are the start rows, sums and counts are not written
            assert np.array_equal(got["centroids"], xb[rows]) and got["untouched"]["sums"] and got["untouched"]["counts"]
            assert got["info"].tolist() == [0, 0, 0, 0]


def test_equal_start_rows_leave_the_second_cluster_empty(engine):
    n, d, kt, k, noise = R.CASES["d64"]
    xb, rows = R.load_case("d64")
    xb = xb.copy()
    xb[rows[1]] = xb[rows[0]]  # two identical rows in the data, both in the start
    for max_iter in (1, 50):
        ref = R.run(xb, xb[rows], max_iter)
        assert ref["gap"] > 4 * R.delta(d)  # the tie between the equal centroids is no gap: their scores are equal bit for bit
        got = _run_raw(engine, xb, k, rows, max_iter)
        _same_run(got, ref, d)
        if max_iter == 1:  # the update saw cluster 1 empty: count 0, sums 0, its centroid row kept
            assert got["counts"][1] == 0 and got["info"][3] == 1 and not got["sums"][1].any() and np.array_equal(got["centroids"][1], xb[rows[1]])
            assert ref["empty"] == 1 and not ref["converged"]
        else:
            assert ref["converged"] and got["info"][2] == 1


def test_every_row_its_own_cluster(engine):
    xb, _ = R.load_case("d64")
    for n in (1, 64, 100):
        x = xb[:n]
        ref = R.run(x, x, 5)
        assert ref["gap"] > 4 * R.delta(64) and ref["iterations"] == 1 and ref["converged"]
        got = _run_raw(engine, x, n, np.arange(n), 5)
        _same_run(got, ref, 64)
        assert got["labels"].tolist() == list(range(n)) and got["counts"].tolist() == [1] * n


# ---- refusals and the Python layer --------------------------------------------------------------------------------------------

def test_refusals_name_the_field_and_leave_the_context_usable(engine):
    from multimodal_embeddings_amd._lib import MmeError, _KmeansState

    xb, rows = R.load_case("d64")
    n, d, k = xb.shape[0], 64, len(rows)
    x = _bf16(xb)
    narrow = _bf16(xb[:, :32].copy())
    good = _run_raw(engine, xb, k, rows, 3)
    bufs = {"centroids": Guarded((k, d), torch.int16), "sums": Guarded((k, d), torch.float64), "counts": Guarded((k,), torch.int32),
            "labels": Guarded((n,), torch.int32), "sim": Guarded((n,), torch.float32), "info": Guarded((4,), torch.int64),
            "objective": Guarded((1,), torch.float64)}

    def call(emb=x, N=n, dd=d, kk=k, init=rows, max_iter=3, null=None, state=True):
        st = _KmeansState()
        for f, g in bufs.items():
            setattr(st, f, None if f == null else g.t.data_ptr())
        r = None if init is None else np.ascontiguousarray(init, dtype=np.int32)
        rc = engine.lib.mme_kmeans(engine.h, None if emb is None else emb.data_ptr(), N, dd, kk, None if r is None else r.ctypes.data, max_iter,
                                   C.byref(st) if state else None, engine._stream())
        return rc, engine.lib.mme_last_error(engine.h).decode()

    twice = rows.copy()
    twice[4] = twice[2]
    outside = rows.copy()
    outside[3] = n
    cases = [(dict(emb=narrow, dd=32), "d = 32"), (dict(dd=0), "d = 0"), (dict(kk=0, init=None), "k = 0"), (dict(kk=n + 1, init=None), f"k = {n + 1}"),
             (dict(N=70000, kk=65537, init=None), "k = 65537"), (dict(max_iter=-1), "max_iter = -1"), (dict(max_iter=1001), "max_iter = 1001"),
             (dict(init=outside), f"init_rows[3] = {n}"), (dict(init=-rows - 1), "init_rows[0] = -"), (dict(init=twice), f"row {twice[2]} twice"),
             (dict(emb=None), "emb is null"), (dict(state=False), "state is null"), (dict(N=0), "N = 0")]
    cases += [(dict(null=f), f"state.{f} is null") for f in bufs]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and "mme_kmeans" in msg and text in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in bufs.values()), kw  # nothing was enqueued
        again = _run_raw(engine, xb, k, rows, 3)  # and the context serves the next call
        assert np.array_equal(again["labels"], good["labels"]) and np.array_equal(again["centroids"], good["centroids"])
    # the single-launch entry refuses by field too
    lab, sim, mv = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    q = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    for kw, text in [(dict(op=3, qsim=q, k=8), "op 3"), (dict(op="argmax", qsim=q, k=9), "k = 9"), (dict(op="argmax", qsim=q, k=6, ld=6), "ld = 6"),
                     (dict(op="argmax", qsim=None, k=8, N=4, ld=8), "qsim"), (dict(op="argmax", qsim=q, k=0), "k = 0"),
                     (dict(op="assign", emb=narrow[:4], centroids=narrow[:2]), "d = 32"), (dict(op="assign", emb=x[:4], centroids=x[:2], chunk_rows=-1), "chunk_rows = -1"),
                     (dict(op="update", emb=x[:4], centroids=x[:2].clone()), "sums")]:
        op = kw.pop("op")
        with pytest.raises(MmeError, match="mme_kmeans_apply") as e:
            engine.kmeans_apply(op, labels=lab, sim=sim, moved=mv, **kw)
        assert text in str(e.value), (kw, str(e.value))
    # Engine.kmeans: its own checks, then the library's through MmeError
    for kw, text in [(dict(), "exactly one"), (dict(init_rows=rows, centroids=x[:k]), "exactly one"), (dict(init_rows=rows[:3]), "init_rows has 3"),
                     (dict(centroids=x[:k].float()), "bfloat16 tensor"), (dict(centroids=x[: k - 1]), "bfloat16 tensor"), (dict(init_rows=twice), "twice")]:
        with pytest.raises(MmeError) as e:
            engine.kmeans(x, k, **kw)
        assert text in str(e.value), (kw, str(e.value))
    with pytest.raises(MmeError, match="2-D bfloat16"):
        engine.kmeans(x.float(), k, init_rows=rows)
    res = engine.kmeans(x, k, init_rows=rows, max_iter=3)
    assert np.array_equal(res.labels.cpu().numpy(), good["labels"]) and np.array_equal(_bits(res.centroids), good["centroids"])
    assert res.info.tolist() == good["info"].tolist() and res.objective.item() == good["objective"][0]


def _blob_collection(seed=0, blobs=4, per=30, d=64, noise=0.02):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    rng = np.random.default_rng(seed)
    centres = np.eye(d)[:blobs] * 1.0
    truth = np.repeat(np.arange(blobs), per)
    order = rng.permutation(blobs * per)
    truth = truth[order]
    emb = centres[truth] + noise * rng.standard_normal((blobs * per, d))
    col = RegionCollection()
    ids = [f"region_{r}" for r in range(len(truth))]
    metas = [{"parent_image": f"/data/pages/page{r % 5}.png", "region_type": "advert", "area_percentage": 2.0, "is_region": True} for r in range(len(truth))]
    col.upsert(ids=ids, embeddings=emb.tolist(), metadatas=metas)
    col.upsert(ids=["page_0"], embeddings=[centres[0].tolist()], metadatas=[{"parent_image": "/data/pages/page0.png", "is_region": False}])
    return col, ids, truth, emb


def test_cluster_regions_returns_the_planted_partition(engine, tmp_path):
    from multimodal_embeddings_amd import region_compare as rc

    col, ids, truth, emb = _blob_collection()
    path = str(tmp_path / "reports" / "clusters.json")
    table = rc.create_region_cluster_report(col, 4, output_path=path, engine=engine)
    with open(path) as fh:
        assert json.load(fh) == table  # the report round-trips
    assert table["n_regions"] == 120 and table["n_clusters"] == 4 and table["n_empty"] == 0 and table["converged"] is True
    assert "page_0" not in {m["id"] for c in table["clusters"] for m in c["members"]}  # the page's own row is no region
    blob_of = dict(zip(ids, truth.tolist()))
    seen = set()
    for c in table["clusters"]:
        blobs = {blob_of[m["id"]] for m in c["members"]}
        assert len(blobs) == 1 and c["size"] == 30 and c["medoid"] == c["members"][0]["id"] and c["cohesion"] > 0.9
        assert [m["score"] for m in c["members"]] == sorted((m["score"] for m in c["members"]), reverse=True)
        assert c["pages"] == [f"page{p}.png" for p in range(5)]
        seen |= blobs
    assert seen == {0, 1, 2, 3}
    # explicit start rows, one of each blob, number the clusters: the same groups in the order given
    first = [int(np.nonzero(truth == b)[0][0]) for b in range(4)]
    t2 = rc.cluster_regions(col, 4, init=np.array(first[::-1]), engine=engine)
    assert [[m["id"] for m in c["members"]] for c in t2["clusters"]] == [[m["id"] for m in c["members"]] for c in sorted(
        table["clusters"], key=lambda c: -blob_of[c["medoid"]])]
    # which existing group does a new region belong to: fewer rows than clusters, and many
    t, arr = rc.kmeans_regions(col, 4, init=np.array(first), engine=engine)
    assert [blob_of[c["medoid"]] for c in t["clusters"]] == [0, 1, 2, 3] and arr["labels"].tolist() == truth.tolist()
    new = np.eye(64)[[2, 0]] + 0.01
    lab, sim = rc.assign_regions(arr["centroids"], new, engine=engine)
    assert lab.tolist() == [2, 0] and lab.dtype == np.int32 and sim.shape == (2,) and (sim > 0.9).all()
    lab, sim = rc.assign_regions(arr["centroids"], emb, engine=engine)
    assert lab.tolist() == truth.tolist() and np.allclose(sim, arr["sim"], atol=1e-6)


def test_n_init_keeps_the_best_of_its_runs(engine):
    from multimodal_embeddings_amd import region_compare as rc

    # overlapping blobs and a random start: the runs end in different optima
    col, ids, truth, emb = _blob_collection(seed=1, blobs=6, per=20, noise=0.15)
    table, arr = rc.kmeans_regions(col, 6, init="random", seed=11, n_init=3, max_iter=50, engine=engine)
    singles = [rc.kmeans_regions(col, 6, init="random", seed=11 + r, n_init=1, max_iter=50, engine=engine) for r in range(3)]
    objs = [s[0]["objective"] for s in singles]
    assert arr["objectives"] == objs and arr["best_run"] == int(np.argmax(objs)) and table["objective"] == max(objs)
    assert table == singles[arr["best_run"]][0]
