"""The MFMA GEMM with each epilogue, the LayerNorm statistics chain and the row kernels of the ViT-B/16 forward, one
launch at a time (mme_gemm_apply, mme_rowop_apply), against float64 written here from the definitions.

Reference: float64 on the device with torch, from the SAME bf16 bits the kernel reads (`acc = A . W^T`, then the
epilogue's formula; LayerNorm two-pass from the definition; erf-GELU `x/2 (1 + erf(x / sqrt 2))`).  Nothing is taken from
kernel code.  Every output element of every case is compared, and every output buffer (bf16 / f32 matrix, partial-sum
planes, statistics) sits between guard rows -- and guard columns where the row pitch exceeds N -- pre-filled with a
sentinel NaN bit pattern that must be unchanged afterwards.  Every GEMM case asserts which kernel ran (`ran_256`).

(a) Exact cases, zero tolerance.  A, W small integers (|a w| <= 9, optionally times a power of two), bias / pos / colsum
    / residual integers, planted dyadic (mean, rstd): every partial sum is an integer below 2^24 (asserted per element
    from the f64 pass: sum |a w| < 2^24), so f32 accumulation is exact in any order and rounding mode and the output is
    bf16_rne(exact value).  Ties (257 -> 256) occur naturally.  Epilogue 8 / 3 planes: f32 of the exact sum and sum of
    squares of the ROUNDED outputs per 64-column slice (entries in -1..1 and K <= 1280 keep these below 2^24, asserted).
(b) Random data.  |got - ref| <= ulp_bf16(ref)/2 + K 2^-23 sum_k |a_k w_k| + 4 * 2^-24 (|acc| + |bias| + |res| + |pos|):
    bf16 products are exact in f32; at most K additions, each with relative error <= 2^-23 whether the matrix pipe
    rounds or truncates; then the epilogue's few f32 operations; the first term is the final rounding (dropped for the
    f32 output).  Loose by design at large K -- the exact cases carry the sharpness.
(c) GELU.  Pre-activations known exactly (one-hot A rows times a bf16 value, W's first column a bf16 value: acc = a w),
    > 10^5 distinct values of [-12, 12], dense in [-6, 0], plus 0, +-2^-100, +-9, +-9.0625, +-100, +-3e38.  Tolerance
    ulp_bf16(ref)/2 (1 + 2^-6) + 3e-5: the fit error gemm_epilogue.h states is 2.6e-5 (2.52e-5 re-checked in f64
    arithmetic, 2.56e-5 in f32 arithmetic, over 2.4 M points); the rest covers the hardware exp2 / rcp.  The interior-tile
    (fast) and the edge-tile (slow, 128 x 128 kernel) epilogues share the tolerance and agree bit for bit.
(d) LayerNorm statistics.  One canonical order: ln_stats_canonical_rows (contiguous, strided, row0 > 0) and
    ln_finish_rows fed by an epilogue-8 launch and by a patch-embed launch agree BIT FOR BIT on the same rows.  Against
    f64 (two-pass), u = 2^-24, n = 18 (a term passes at most 16 dot2 accumulation steps and 2 combining adds in f32
    before the f64 sum):  |mean - mean_ref| <= n u sum|x| / d + 2^-24 |mean_ref|;
    |var - var_ref| <= n u (sum x^2 / d + 2 |mean_ref| sum|x| / d) + (n u sum|x| / d)^2 + 2^-22 (var_ref + eps), with
    var = rstd^-2 - eps recovered in f64 from the returned f32 rstd (the last term is that rounding).  The bound scales
    with sum x^2 / d, not with the variance: for rows whose mean is large against their spread (the "+30" family:
    bound 2.9e-3 of a variance of ~1; an offset of 2^10 with unit spread would give a bound above the variance, and
    there the bf16 step of the data, 2^3, already exceeds the spread) it only says that the one-pass form loses no more
    than f32 slice sums must.  Constant rows: every sum is exact, var == 0 and rstd == float32(1 / sqrt(eps)) bit for bit
    (eps 1e-12 and 1e-5).  Observed error / bound, maximum per family (MI355X; printed by the test):
    (not recorded yet: the test prints them per family, `pytest -s`; a numpy emulation of the canonical order with f32
    partial sums stays below 5 % of the bound on every family.)
    Two-pass f32 kernels (ln_stats_rows, layernorm_rows; d = 768).  A two-pass form computes
    q = sum (x - m)^2 = sum (x - mean)^2 + d (mean - m)^2 with every f32 sum of d terms off by at most d 2^-24 relative
    to the sum of the magnitudes, and 1 / d rounded once; with e = d 2^-23:  |mean - mean_ref| <= e sum|x| / d,
    |var - var_ref| <= e var_ref + (e sum|x| / d)^2 + 2^-22 (var_ref + eps)  (relative to the scale of each quantity),
    output within ulp_bf16(ref)/2 + e ((|x| + |mean|) rstd |gamma| + |beta|).
    Composition as the forward runs it: canonical statistics -> epilogue 5 with W' = bf16(W gamma), colsum =
    f32(sum_k W'), b' = f32(b + W . beta) (f64 sums) against f64 LayerNorm(x) . W'^T + b'.  With
    out = rstd (acc - mean colsum) + b':  an accumulation error d_acc <= K 2^-23 sum|x w'| enters times rstd; a mean error
    d_mean enters as d_mean |colsum| rstd; a relative rstd error enters times |out - b'|; plus the final rounding:
    tol = ulp_bf16(ref)/2 + rstd K 2^-23 sum|x w'| + d_mean |colsum| rstd + (d_rstd / rstd) |ref - b'|, with d_mean and
    d_var the canonical bounds above and d_rstd / rstd = d_var / (2 (var + eps)) + 2^-24.
(e) Row kernels.  cls_rows: bf16_rne(f32(cls + pos[0])) bit for bit on rows b*197 only.  pool_ln_l2: bf16 output == RNE
    of the f32 output bit for bit; f32 output against f64 within 8 x the maximum deviation of a plain float32 numpy
    restatement of the same definition from f64 on the same inputs (another summation order), never below 2^-22.
    Measured: float32 yardstick 1.97e-8 / 3.58e-8 / 1.84e-8 (tokens 0 / 77 / 196; tolerance 2.4e-7 / 2.9e-7 / 2.4e-7); the
    kernel's observed maximum is printed by the test (`pytest -s`; not recorded yet).  A zero row gives beta / ||beta||.
(f) Sharpness.  Each family names mutants -- plausible kernel bugs written as changes of the REFERENCE -- and asserts
    that each differs from the true reference in bits (exact families) or by more than 4 x the tolerance on a stated
    minimum number of elements: the two column blocks of a permlane16_swap pair exchanged; residual from row m + 16;
    rows 112..127 of every 128-row wave tile (the deferred block) left at their previous contents; the last K-tile
    dropped; patch rows mapped without the +1 per crop; pos[p] for pos[1 + p]; colsum ignored; plane slice index off by
    one; bias added after GELU; tanh-GELU; rstd from Q/d without - mean^2.
(g) Argument validation: each documented precondition returns MME_E_ARG (MmeError) with its message, and the
    sentinel-filled output is untouched.  Only invalid-argument returns are exercised.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NP, T = 196, 197          # patches / tokens per crop
SENT16 = 0x7FA5           # bf16 NaN
SENT32 = 0x7FA5A5A5       # f32 NaN
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0**-24


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, amax, g, dtype=F64):
    return torch.randint(-amax, amax + 1, shape, generator=g, device=DEV).to(dtype)


def _randn(shape, g, scale=1.0, dtype=F32):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


class Guard:
    """rows x ld elements between `guard` rows of sentinel; the valid block is [:, :n], the rest of each row is guard too."""

    def __init__(self, dtype, rows, n, ld=None, guard=3):
        if ld is None:  # bf16 rows are stored 16 bytes at a time: the pitch is N rounded up to 8 (guard columns where N % 8 != 0)
            ld = -(-n // 8) * 8 if dtype == BF16 else n
        self.rows, self.n, self.ld, self.g = rows, n, ld, guard
        self.bits, self.sent = (torch.int16, SENT16) if dtype == BF16 else (torch.int32, SENT32)
        self.raw = torch.full(((rows + 2 * guard) * self.ld,), self.sent, dtype=self.bits, device=DEV)
        self.view = self.raw.view(dtype).view(rows + 2 * guard, self.ld)[guard : guard + rows]  # what the kernel gets
        self.valid = self.view[:, :n]

    def valid_bits(self):
        return self.raw.view(self.rows + 2 * self.g, self.ld)[self.g : self.g + self.rows, : self.n]

    def check(self, what):
        b = self.raw.view(self.rows + 2 * self.g, self.ld)
        ok = bool((b[: self.g] == self.sent).all()) and bool((b[self.g + self.rows :] == self.sent).all())
        ok = ok and bool((b[:, self.n :] == self.sent).all())
        assert ok, f"{what}: guard region overwritten"

    def untouched(self):
        return bool((self.raw == self.sent).all())


def expect_256(variant, M, N, K):
    """Which kernel a launch must run (include/mme.h): K = 64 and variant 1 -> 128 x 128; 0 = by tile count."""
    if K < 128 or variant == 1:
        return False
    if variant == 0:
        return -(-M // 256) * -(-N // 256) >= 128
    return True


def acc64(A, W):
    return A.double() @ W.double().T


def absacc64(A, W):
    return A.double().abs() @ W.double().abs().T


def token_rows(M):
    """patch row m = (crop b, patch p) -> token row b*197 + 1 + p, from the definition"""
    m = torch.arange(M, device=DEV)
    return (m // NP) * T + 1 + (m % NP)


def ulp_bf16(x):
    """spacing of bf16 at |x| (f64 in, f64 out); 0 at 0"""
    _, e = torch.frexp(x.abs())
    u = torch.ldexp(torch.ones_like(x), e - 8).clamp_min(2.0**-133)
    return torch.where(x == 0, torch.zeros_like(x), u)


def rne_bf16_bits(x64, what):
    """bits of bf16_rne(x) for f64 values that f32 holds exactly (asserted: no double rounding)"""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), f"{what}: an expected value is not exact in f32"
    return x32.to(BF16).view(torch.int16)


def launch(eng, epi, A, W, variant, *, reverse_m=0, bias=None, res=None, inplace=True, pos=None, ln_stats=None, colsum=None, ld=None,
           planes=False, what=""):
    """One guarded launch.  -> (valid output block (bf16 or f32 view), planes [2, N/64, R] or None, ran_256)"""
    M, K = A.shape
    N = W.shape[0]
    rows = M // NP * T if epi == 3 else M
    kw = {}
    if epi == 4:
        buf = Guard(F32, rows, N, ld)
        kw.update(outf=buf.view, ldf=buf.ld)
    else:
        buf = Guard(BF16, rows, N, ld)
        kw.update(out=buf.view, ldo=buf.ld, bias=bias)
    if res is not None:
        if inplace:
            buf.valid.copy_(res)
            kw["res"] = buf.view
        else:
            rb = torch.zeros((rows, buf.ld), dtype=BF16, device=DEV)
            rb[:, :N] = res
            kw["res"] = rb
    pb = None
    if planes:
        R = rows + 5
        pb = Guard(F32, 1, 2 * (N // 64) * R, guard=64)
        kw.update(ln_part=pb.view, ln_part_rows=R)
    ran = eng.gemm_apply(epi, A, W, variant=variant, reverse_m=reverse_m, pos=pos, ln_stats=ln_stats, colsum=colsum, **kw)
    want = expect_256(variant, M, N, K)
    assert ran == want, f"{what}: ran_256 = {ran}, expected {want} (variant {variant}, M {M}, N {N}, K {K})"
    buf.check(what)
    if pb is not None:
        pb.check(what + " (planes)")
    if res is not None and not inplace:
        assert torch.equal(rb[:, :N].view(torch.int16), res.view(torch.int16)), f"{what}: the out-of-place residual was modified"
    return buf.valid, (pb.valid.view(2, N // 64, -1) if pb is not None else None), ran


def assert_bits(got, want, what):
    if not torch.equal(got, want):
        bad = got != want
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits; first at {first}: "
                             f"got {int(got[tuple(first)]) & 0xFFFFFFFF:#x} want {int(want[tuple(first)]) & 0xFFFFFFFF:#x}; "
                             f"rows affected {int(bad.any(1).sum())}, columns affected {int(bad.any(0).sum())}")


def assert_close(got64, ref, tol, what):
    fin = torch.isfinite(got64)
    assert bool(fin.all()), f"{what}: {int((~fin).sum())} non-finite outputs, first at {(~fin).nonzero()[0].tolist()}"
    err = (got64 - ref).abs()
    bad = err > tol
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: max err / tol = {ratio:.3g}")
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs out of tolerance (worst err / tol {ratio:.3g}); first at {list(i)}: "
                             f"got {float(got64[i])!r} ref {float(ref[i])!r} tol {float(tol[i])!r}")


def assert_mutant_bits(mut, want, least, name):
    n = int((mut != want).sum())
    assert n >= least, f"mutant '{name}' differs from the reference in {n} elements only (< {least}): the case would not catch it"


def assert_mutant_far(mut, ref, tol, least, name):
    n = int(((mut - ref).abs() > 4 * tol).sum())
    assert n >= least, f"mutant '{name}' leaves 4 x the tolerance on {n} elements only (< {least}): the case would not catch it"


# ---------------------------------------------------------------------------------------------------------------------
# (a) exact cases


def exact_inputs(epi, M, N, K, seed, amax=3, scale=(1.0, 1.0)):
    g = _gen(seed)
    d = {"A": (_ints((M, K), amax, g) * scale[0]).to(BF16), "W": (_ints((N, K), amax, g) * scale[1]).to(BF16)}
    rows = M // NP * T if epi == 3 else M
    if epi != 4:
        d["bias"] = _ints((N,), 50, g, F32)
    if epi in (2, 8):
        d["res"] = _ints((rows, N), 100 if amax > 1 else 2, g, BF16)
    if epi == 3:
        d["pos"] = _ints((T, N), 60 if amax > 1 else 2, g, F32)
    if epi == 5:
        mean = torch.tensor([0.0, 0.5, -0.5, 3.0], device=DEV)[torch.randint(0, 4, (M,), generator=g, device=DEV)]
        rstd = torch.tensor([0.25, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (M,), generator=g, device=DEV)]
        d["ln_stats"] = torch.stack([mean, rstd], 1).contiguous()
        d["colsum"] = _ints((N,), 200, g, F32)
    return d


def exact_value(epi, d, acc=None, unit=1.0):
    """f64 value of every output element before the final rounding, [M, N] by GEMM row; asserts exactness of the accumulation"""
    A, W = d["A"], d["W"]
    bound = absacc64(A, W)
    assert float(bound.max()) < 2.0**24 * unit, "sum |a w| reaches 2^24: accumulation not exact in every order"
    acc = acc64(A, W) if acc is None else acc
    if epi == 4:
        return acc
    v = acc + d["bias"].double()
    if epi in (2, 8):
        v = v + d["res"].double()
    if epi == 3:
        p = torch.arange(A.shape[0], device=DEV) % NP
        v = v + d["pos"].double()[1 + p]
    if epi == 5:
        st = d["ln_stats"].double()
        v = st[:, 1:2] * (acc - st[:, 0:1] * d["colsum"].double()) + d["bias"].double()
    return v


def expected_bits(epi, d, value, what):
    """bit image of the whole valid output block (patch embed: [CLS] rows keep the sentinel)"""
    if epi == 4:
        assert torch.equal(value.float().double(), value)
        return value.float().view(torch.int32)
    b = rne_bf16_bits(value, what)
    if epi != 3:
        return b
    M = value.shape[0]
    full = torch.full((M // NP * T, value.shape[1]), SENT16, dtype=torch.int16, device=DEV)
    full[token_rows(M)] = b
    return full


def expected_planes(out_bits, rows_idx, what):
    """f32 (sum, sum of squares) of the rounded outputs per 64-column slice: [2, N/64, len(rows_idx)]"""
    o = out_bits[rows_idx].view(BF16).double()
    o = o.view(o.shape[0], -1, 64)
    s, q = o.sum(-1), (o * o).sum(-1)
    assert float(q.max()) < 2.0**24 and float(s.abs().max()) < 2.0**24, f"{what}: slice sums not exact in f32"
    return torch.stack([s.T, q.T]).float()


def t_int_formula(M):
    """stem's t_int (csrc/image_tower.hip): one past the last token row an interior patch tile covered"""
    interior = M // 256 * 256
    return interior - 1 + (interior - 1) // NP + 2 if interior else 0


def row_tile(epi, variant):
    """Row-tile height of the large-tile kernel an explicit `variant` resolves to (include/mme.h): 384 under variant 6 for the
    epilogues the 384 x 256 kernel is built for (0, 1, 2, 5, 6, 8), else 256 (epilogues 3 and 4 resolve to variant 4)."""
    return 384 if variant == 6 and epi in (0, 1, 2, 5, 6, 8) else 256


def check_planes(epi, planes, out_bits, M, N, ran, what, tm=256):
    """`tm`: the row-tile height of the kernel that ran (row_tile): the planes are promised for the rows of its interior row tiles"""
    if not ran:
        assert bool(torch.isnan(planes).all()), f"{what}: the 128 x 128 kernel wrote partial-sum planes"
        return
    interior = M // tm * tm
    m = torch.arange(interior, device=DEV)
    rows_idx = token_rows(interior) if epi == 3 else m
    if N % 256 == 0 and interior:
        want = expected_planes(out_bits, rows_idx, what)
        assert_bits(planes[:, :, rows_idx].contiguous().view(torch.int32).flatten(0, 1), want.view(torch.int32).flatten(0, 1), what + " planes")
        # mutant: slice index off by one
        assert_mutant_bits(torch.roll(want, 1, 1).view(torch.int32), want.view(torch.int32), want.numel() // 2, "plane slice index off by one")
    if epi == 3:
        written = (~torch.isnan(planes[0, 0])).nonzero().flatten()
        assert torch.equal(written, rows_idx), f"{what}: the token rows with planes are not those of the interior patch tiles"
        t_int = t_int_formula(M)
        r = torch.arange(t_int, device=DEV)
        assert torch.equal(r[r % T != 0], rows_idx), f"{what}: t_int = {t_int} does not delimit the rows the interior tiles wrote"
        for s in range(planes.shape[1]):
            for k in range(2):
                assert torch.equal((~torch.isnan(planes[k, s])).nonzero().flatten(), rows_idx), f"{what}: plane {k} slice {s} covers other rows"


# (epilogue, M, N, K, options).  Properties covered -- kernel: variants 1, 3, 4, 6 always (6 is the 384 x 256 kernel for epilogues
# 0, 2, 5, 8 and variant 4 for 3 and 4; its planes cover 384-row interior tiles), 0 and reverse_m where listed;
# M: 1, 127, 128, 129, 255, 256, 257, ragged last row tiles, 256 and 257 tiles (the persistent loop's has_next boundary at a
# grid of 256), 288 tiles (every workgroup defers into a following tile and flushes a last one); N: 768, 1280, 2304, 3072,
# 3840, 5120, N % 256 != 0 (260, 320, 1028, 261), N < 128; K: 64 (128 x 128 kernel whatever the variant), 128, 192, 640, 768,
# 1280, 3072, 5120; residual in place and out of place; row pitch == N wherever N % 8 == 0 (the 16-byte stores of the interior
# tiles need ldo % 8 == 0, so N = 100, 260, 1028 run with the next multiple of 8 and guard columns), > N for one more bf16 and two
# f32 outputs.
EXACT = [
    (0, 1, 64, 64, {}),
    (0, 127, 260, 128, {"dropk": True}),
    (0, 128, 100, 640, {}),
    (0, 257, 2304, 768, {"swap": True}),
    (0, 5988, 3072, 768, {"extra": [(0, 0), (4, 1), (3, 1)]}),
    (0, 65536, 256, 128, {"extra": [(0, 0)]}),
    (0, 65537, 256, 128, {"extra": [(0, 0)], "dropk": True}),
    (0, 300, 1280, 192, {"scale": (2.0**-3, 2.0**4), "dropk": True}),
    (2, 129, 1028, 192, {}),
    (2, 256, 768, 3072, {"res16": True, "stale": True}),
    (2, 255, 1280, 5120, {"inplace": False}),
    (2, 1100, 768, 768, {"ld": 776, "extra": [(4, 1)], "stale": True}),
    (4, 128, 5120, 1280, {}),
    (4, 513, 1028, 640, {"ld": 1032}),
    (4, 300, 261, 128, {"ld": 263}),
    (4, 1024, 768, 768, {"extra": [(4, 1)]}),
    (5, 256, 2304, 768, {"nocolsum": True}),
    (5, 257, 3840, 1280, {}),
    (5, 127, 100, 64, {}),
    (8, 1101, 768, 768, {"amax": 1, "planes": True, "extra": [(4, 1)]}),
    (8, 512, 1280, 1280, {"amax": 1, "planes": True, "inplace": False}),
    (8, 300, 320, 128, {"amax": 1, "planes": False}),
    (3, 64 * NP, 768, 768, {"amax": 1, "planes": True, "extra": [(0, 0), (3, 1)], "patchmap": True}),
    (3, 50 * NP, 768, 768, {"amax": 1, "planes": True}),
    (3, 3 * NP, 768, 768, {"patchmap": True}),
    (3, 2 * NP, 1280, 128, {"planes": True, "amax": 1}),
]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: f"epi{c[0]}-M{c[1]}-N{c[2]}-K{c[3]}")
def test_exact_bit_for_bit(eng, case):
    epi, M, N, K, opt = case
    what = f"exact epilogue {epi} M {M} N {N} K {K}"
    scale = opt.get("scale", (1.0, 1.0))
    d = exact_inputs(epi, M, N, K, 7000 + 13 * M + N + K + epi, amax=opt.get("amax", 3), scale=scale)
    unit = scale[0] * scale[1]
    value = exact_value(epi, d, unit=unit)
    want = expected_bits(epi, d, value, what)
    planes_on = opt.get("planes", epi == 8)
    # epilogue 8 always takes a plane buffer; "planes": False only says that N % 256 != 0 leaves no complete row to compare
    give_planes = epi == 8 or (epi == 3 and planes_on)
    runs = [(1, 0), (3, 0), (4, 0), (6, 0)] + opt.get("extra", [])
    for variant, rev in runs:
        w = f"{what} variant {variant} reverse {rev}"
        out, planes, ran = launch(eng, epi, d["A"], d["W"], variant, reverse_m=rev, bias=d.get("bias"), res=d.get("res"),
                                  inplace=opt.get("inplace", True), pos=d.get("pos"), ln_stats=d.get("ln_stats"), colsum=d.get("colsum"),
                                  ld=opt.get("ld"), planes=give_planes, what=w)
        got = out.view(torch.int32 if epi == 4 else torch.int16)
        assert_bits(got, want, w)
        if give_planes:
            check_planes(epi, planes, want, M, N, ran, w, tm=row_tile(epi, variant))
    # ---- sharpness: each mutant is a change of the reference that this case's comparison would see
    if opt.get("swap"):  # the two 8-column blocks a permlane16_swap pair exchanges: columns 32q + 8..15 <-> 32q + 16..23
        c = torch.arange(N, device=DEV)
        r = c % 32
        perm = torch.where((r >= 8) & (r < 16), c + 8, torch.where((r >= 16) & (r < 24), c - 8, c))
        assert_mutant_bits(want[:, perm], want, want.numel() // 4, "permlane16_swap pair exchanged")
    if opt.get("res16"):  # residual taken from row m + 16
        dm = dict(d)
        dm["res"] = torch.roll(d["res"], -16, 0)
        assert_mutant_bits(rne_bf16_bits(exact_value(epi, dm), what), want, want.numel() // 2, "residual from row m + 16")
    if opt.get("stale"):  # the deferred row block (rows 112..127 of each 128-row wave tile) left at its previous contents
        m = torch.arange(M, device=DEV)
        stale = (m % 128) >= 112
        mut = want.clone()
        mut[stale] = d["res"].view(torch.int16)[stale]
        assert_mutant_bits(mut, want, int(stale.sum()) * N // 2, "deferred row block not stored")
    if opt.get("dropk"):  # the last K-tile dropped
        mv = exact_value(epi, d, acc=acc64(d["A"][:, : K - 64], d["W"][:, : K - 64]), unit=unit)
        assert_mutant_bits(rne_bf16_bits(mv, what), want, want.numel() // 2, "last K-tile dropped")
    if opt.get("nocolsum"):  # colsum ignored
        dm = dict(d)
        dm["colsum"] = torch.zeros_like(d["colsum"])
        assert_mutant_bits(rne_bf16_bits(exact_value(epi, dm), what), want, want.numel() // 3, "colsum ignored")
    if opt.get("patchmap"):
        b = rne_bf16_bits(value, what)
        mut = torch.full_like(want, SENT16)
        mut[torch.arange(M, device=DEV) + 1] = b  # rows mapped without the +1 per crop
        assert_mutant_bits(mut, want, (M - NP) * N // 2, "patch rows mapped without the +1 per crop")
        dm = dict(d)
        dm["pos"] = torch.roll(d["pos"], 1, 0)  # pos[p] for pos[1 + p]
        assert_mutant_bits(expected_bits(epi, dm, exact_value(epi, dm), what), want, M * N // 3, "pos[p] for pos[1 + p]")


# ---------------------------------------------------------------------------------------------------------------------
# (b) random data

RANDOM = [
    (0, 300, 2304, 768, 1.0, {}),
    (0, 257, 260, 64, 1.0, {}),
    (2, 515, 768, 3072, 1.0, {}),
    (2, 256, 1280, 5120, 2.0**-6, {"inplace": False}),
    (3, 3 * NP, 768, 768, 1.0, {}),
    (4, 257, 1028, 5120, 2.0**6, {}),
    (4, 512, 768, 768, 1.0, {}),
    (8, 512, 768, 768, 1.0, {}),
    (0, 2 * 256 + 9, 3840, 1280, 1.0, {}),
    (0, 256, 5120, 1280, 1.0, {}),
    (2, 1536, 3072, 640, 1.0, {}),
]


@pytest.mark.parametrize("case", RANDOM, ids=lambda c: f"epi{c[0]}-M{c[1]}-N{c[2]}-K{c[3]}-x{c[4]:g}")
def test_random_rounding_level(eng, case):
    epi, M, N, K, sc, opt = case
    what = f"random epilogue {epi} M {M} N {N} K {K} scale {sc:g}"
    g = _gen(9000 + M + N + K + epi)
    A, W = _randn((M, K), g, sc, BF16), _randn((N, K), g, sc, BF16)
    rows = M // NP * T if epi == 3 else M
    bias = _randn((N,), g) if epi != 4 else None
    res = _randn((rows, N), g, 1.0, BF16) if epi in (2, 8) else None
    pos = _randn((T, N), g) if epi == 3 else None
    acc, aab = acc64(A, W), absacc64(A, W)
    ref, mag = acc.clone(), acc.abs()
    if bias is not None:
        ref += bias.double()
        mag += bias.double().abs()
    if res is not None:
        ref += res.double()
        mag += res.double().abs()
    if pos is not None:
        p = pos.double()[1 + torch.arange(M, device=DEV) % NP]
        ref += p
        mag += p.abs()
    tol = K * 2.0**-23 * aab + 4 * U * mag
    if epi != 4:
        tol = tol + ulp_bf16(ref) / 2
    outs = []
    for variant in (1, 3, 4):
        w = f"{what} variant {variant}"
        out, planes, ran = launch(eng, epi, A, W, variant, bias=bias, res=res, inplace=opt.get("inplace", True), pos=pos, planes=epi == 8, what=w)
        if epi == 3:
            cls = out[torch.arange(M // NP, device=DEV) * T].view(torch.int16)
            assert bool((cls == SENT16).all()), f"{w}: a [CLS] row was written"
            out = out[token_rows(M)]
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    for o in outs[1:]:  # same MFMA instruction, same K order per output element (include/mme.h)
        assert torch.equal(o.view(torch.int32 if epi == 4 else torch.int16), outs[0].view(torch.int32 if epi == 4 else torch.int16)), f"{what}: variants differ in bits"
    mut = ref - acc + acc64(A[:, : K - 64], W[:, : K - 64]) if K > 64 else None
    if mut is not None and K <= 768:
        assert_mutant_far(mut, ref, tol, ref.numel() // 2, "last K-tile dropped")


# ---------------------------------------------------------------------------------------------------------------------
# (c) GELU


def gelu_ref(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x**3)))


def gelu_tol(ref):
    return ulp_bf16(ref) / 2 * (1 + 2.0**-6) + 3e-5


def _bf16_from_bits(lo, hi, step=1):
    return torch.arange(lo, hi, step, device=DEV, dtype=torch.int32).to(torch.int16).view(BF16).double()


def gelu_grid():
    """A [1024, 128] with two entries per row (a_m, c_m), W [256, 128] with first columns (w_n, v_n): acc[m, n] = a_m w_n + c_m v_n,
    two products whose sum f32 holds exactly (asserted).  a: every bf16 value of [-12, -0.25], every third of [0.25, 12], small
    negatives, the listed special values; w: 256 values of [0.25, 1); c v: multiples of 2^-12 below 2^-7 that break the
    product structure (only ~8000 distinct 8-bit x 8-bit mantissa products exist per binade)."""
    M, N, K = 1024, 256, 128
    special = torch.tensor([0.0, -0.0, 2.0**-100, -(2.0**-100), 9.0, -9.0, 9.0625, -9.0625, 100.0, -100.0, 3e38, -3e38], dtype=F64, device=DEV)
    a = torch.cat([
        -_bf16_from_bits(0x3E80, 0x4140),           # [-12, -0.25]: 704 values, all of bf16 there
        _bf16_from_bits(0x3E80, 0x4141, 3),         # [0.25, 12]: 235 values
        -_bf16_from_bits(0x3D00, 0x3D00 + 4 * 73, 4),  # 73 values of (-0.25, -0.03]
        special,
    ]).to(BF16)
    assert a.numel() == M
    c = 2.0**-9 * (1 + torch.arange(M, device=DEV) % 4).double()
    c[M - special.numel() :] = 0.0  # the listed values stay themselves
    n = torch.arange(N, device=DEV, dtype=F64)
    w = torch.where(n < 128, 0.5 + n / 256, 0.25 + (n - 128) / 512)
    w[255] = 1.0
    v = (n % 8) / 8
    v[255] = 0.0
    A = torch.zeros((M, K), dtype=BF16, device=DEV)
    W = torch.zeros((N, K), dtype=BF16, device=DEV)
    A[:, 0], A[:, 1] = a, c.to(BF16)
    W[:, 0], W[:, 1] = w.to(BF16), v.to(BF16)
    W[:, 2:] = 1.0  # met by zeros of A only
    assert torch.equal(W[:, 0].double(), w) and torch.equal(A[:, 1].double(), c)
    return A, W, a.double()[:, None] * w[None, :] + c[:, None] * v[None, :]


@pytest.mark.parametrize("epi", [1, 6])
def test_gelu_dense_grid_fast_and_slow_path(eng, epi):
    A, W, x = gelu_grid()
    M, N = x.shape
    assert torch.equal(acc64(A, W), x) and torch.equal(x.float().double(), x)
    core = x[(x.abs() <= 12)]
    assert int(torch.unique(core).numel()) >= 100_000, "fewer than 10^5 distinct pre-activations in [-12, 12]"
    assert int(torch.unique(core[(core >= -6) & (core <= 0)]).numel()) >= 30_000
    for v in (0.0, 2.0**-100, 9.0, 9.0625, 100.0):
        assert bool((x == v).any()) and bool((x == -v).any()), v
    assert bool((x.abs() > 2.9e38).any())
    bias = torch.zeros(N, dtype=F32, device=DEV)
    kw = {}
    if epi == 6:
        st = torch.zeros((M, 2), dtype=F32, device=DEV)
        st[:, 1] = 1.0
        kw = dict(ln_stats=st, colsum=torch.zeros(N, dtype=F32, device=DEV))
    ref = gelu_ref(x)
    tol = gelu_tol(ref)
    outs = {}
    for variant in (1, 3, 4):
        w = f"GELU epilogue {epi} variant {variant}"
        out, _, ran = launch(eng, epi, A, W, variant, bias=bias, what=w, **kw)
        assert ran == (variant != 1)  # 3, 4: four interior 256 x 256 tiles (fast path); 1: epi_store (slow path)
        assert_close(out.double(), ref, tol, w)
        outs[variant] = out.clone()
    assert torch.equal(outs[1].view(torch.int16), outs[3].view(torch.int16)), "slow-path and fast-path GELU differ in bits"
    assert torch.equal(outs[4].view(torch.int16), outs[3].view(torch.int16))
    assert_mutant_far(gelu_tanh(x), ref, tol, 2000, "tanh-GELU")
    # K = 64 routes to the 128 x 128 kernel whatever the variant
    out, _, ran = launch(eng, epi, A[:, :64].contiguous(), W[:, :64].contiguous(), 3, bias=bias, what="GELU K = 64", **kw)
    assert not ran
    assert torch.equal(out.view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("epi", [1, 6])
def test_gelu_takes_the_bias_first(eng, epi):
    """x = a_m + bias[n] exactly: a multiples of 2^-4 below 16, bias multiples of 2^-6 in [-2, 2)."""
    M, N, K = 512, 256, 128
    a = ((torch.arange(M, device=DEV, dtype=F64) - 256) / 16).to(BF16)
    bias = ((torch.arange(N, device=DEV, dtype=F64) - 128) / 64).float()
    A = torch.zeros((M, K), dtype=BF16, device=DEV)
    W = torch.zeros((N, K), dtype=BF16, device=DEV)
    A[:, 0] = a
    W[:, 0] = 1.0
    x = a.double()[:, None] + bias.double()[None, :]
    assert torch.equal(x.float().double(), x)
    kw = {}
    if epi == 6:
        st = torch.zeros((M, 2), dtype=F32, device=DEV)
        st[:, 1] = 1.0
        kw = dict(ln_stats=st, colsum=torch.zeros(N, dtype=F32, device=DEV))
    ref = gelu_ref(x)
    tol = gelu_tol(ref)
    outs = []
    for variant in (1, 3, 4):
        w = f"GELU + bias epilogue {epi} variant {variant}"
        out, _, _ = launch(eng, epi, A, W, variant, bias=bias, what=w, **kw)
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16))
    assert_mutant_far(gelu_ref(a.double()[:, None] + 0 * x) + bias.double()[None, :], ref, tol, ref.numel() // 2, "bias added after GELU")
    assert_mutant_far(gelu_tanh(x), ref, tol, 2000, "tanh-GELU")


# ---------------------------------------------------------------------------------------------------------------------
# (d) LayerNorm statistics

FAMILIES = ("normal", "offset30", "massive", "constant", "large", "small")


def ln_rows(d, seed):
    """196 bf16 rows of d (one crop's worth of patch rows) and {family: row indices}"""
    g = _gen(seed)
    fam = {"normal": range(0, 40), "offset30": range(40, 80), "massive": range(80, 120), "constant": range(120, 126), "large": range(126, 166),
           "small": range(166, 196)}
    X = torch.randn((NP, d), generator=g, device=DEV, dtype=F64)
    X[40:80] += 30.0
    for r in fam["massive"]:
        c = torch.randperm(d, generator=g, device=DEV)[:2]
        X[r, c[0]] = 200.0 + 800.0 * float(torch.rand((), generator=g, device=DEV))
        X[r, c[1]] = -(200.0 + 800.0 * float(torch.rand((), generator=g, device=DEV)))
    for r, cval in zip(fam["constant"], (0.0, 1.5, -40.0, 0.0, 1.5, -40.0)):
        X[r] = cval
    X[126:166] = (X[126:166] * 2.0**13).clamp(-(2.0**15), 2.0**15)
    X[166:] *= 2.0**-6
    return X.to(BF16), {k: torch.tensor(list(v), device=DEV) for k, v in fam.items()}


def stats_ref(X):
    x = X.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, var


def canonical_bounds(X, eps):
    """(d_mean, d_var) of the module docstring, per row"""
    x = X.double()
    d = x.shape[1]
    n = 18
    mean, var = stats_ref(X)
    sa, sq = x.abs().sum(1), (x * x).sum(1)
    d_mean = n * U * sa / d + U * mean.abs()
    d_var = n * U * (sq / d + 2 * mean.abs() * sa / d) + (n * U * sa / d) ** 2 + 2.0**-22 * (var + eps)
    return d_mean, d_var


def run_stats(eng, op, rows_total, **kw):
    """a statistics launch into a guarded [rows_total, 2] f32 buffer -> the buffer (NaN sentinel where nothing was written)"""
    st = Guard(F32, rows_total, 2)
    eng.rowop_apply(op, stats=st.view, **kw)
    st.check(op)
    return st.valid.clone()


def f32_eps(eps):
    return float(np.float32(eps))


@pytest.mark.parametrize("d", [768, 1280])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_ln_statistics_chain(eng, d, eps):
    X, fam = ln_rows(d, 4242 + d)
    e32 = f32_eps(eps)
    # ---- stand-alone canonical kernel on the 196 rows: the yardstick of the bit-for-bit comparisons
    can = run_stats(eng, "ln_stats_canonical", NP, x=X, row0=0, row1=NP, d=d, eps=eps)
    assert bool(torch.isfinite(can).all())
    # ---- (1) epilogue 8: out = bf16(0 + 0 + res) = res, planes of the rows of two interior tiles and a ragged one
    M = 600
    idx = torch.arange(M, device=DEV) % NP
    Xr = X[idx].contiguous()
    g = _gen(5)
    A0 = torch.zeros((M, 128), dtype=BF16, device=DEV)
    Wr = _randn((d, 128), g, 1.0, BF16)
    zb = torch.zeros(d, dtype=F32, device=DEV)
    for variant in (3, 4):
        out, planes, ran = launch(eng, 8, A0, Wr, variant, bias=zb, res=Xr, planes=True, what=f"statistics feed, epilogue 8 variant {variant}")
        assert ran and torch.equal(out.view(torch.int16), Xr.view(torch.int16))
        R = planes.shape[2]
        fin = run_stats(eng, "ln_finish", M, part=planes, part_rows=R, rows=512, d=d, eps=eps)
        assert_bits(fin[:512].view(torch.int32), can[idx[:512]].view(torch.int32), f"ln_finish_rows after epilogue 8 (variant {variant}) vs ln_stats_canonical_rows")
        assert bool((fin[512:].view(torch.int32) == SENT32).all()), "ln_finish_rows wrote past `rows`"
    # ---- (2) patch embed: out = bf16(0 + 0 + pos[1 + p]) = X[p]; 3 crops = 588 patch rows, 512 of them in interior tiles
    pos = torch.zeros((T, d), dtype=F32, device=DEV)
    pos[1:] = X.float()
    Ap = torch.zeros((3 * NP, 128), dtype=BF16, device=DEV)
    out, planes, ran = launch(eng, 3, Ap, Wr, 3, bias=zb, pos=pos, planes=True, what="statistics feed, patch embed")
    assert ran
    tok = token_rows(3 * NP)
    assert torch.equal(out[tok].view(torch.int16), X[torch.arange(3 * NP, device=DEV) % NP].view(torch.int16))
    t_int = t_int_formula(3 * NP)
    fin = run_stats(eng, "ln_finish", 3 * T, part=planes, part_rows=planes.shape[2], rows=t_int, d=d, eps=eps)
    covered = token_rows(512)
    assert int(covered.max()) + 1 == t_int
    assert_bits(fin[covered].view(torch.int32), can[torch.arange(512, device=DEV) % NP].view(torch.int32), "ln_finish_rows after the patch embed vs ln_stats_canonical_rows")
    # ---- (3) the stand-alone kernel on that token buffer: a contiguous range with row0 > 0, and every 197th row from row0 > 0
    xt = out.clone().contiguous()  # [3 * 197, d]; [CLS] rows hold the sentinel NaN and are not selected below
    part = run_stats(eng, "ln_stats_canonical", 3 * T, x=xt, row0=T + 1, row1=2 * T, d=d, eps=eps)
    assert_bits(part[T + 1 : 2 * T].view(torch.int32), can.view(torch.int32), "ln_stats_canonical_rows, contiguous from row0 > 0")
    assert bool((part[: T + 1].view(torch.int32) == SENT32).all()) and bool((part[2 * T :].view(torch.int32) == SENT32).all())
    strided = run_stats(eng, "ln_stats_canonical", 3 * T, x=xt, row0=6, row1=3 * T, stride=T, d=d, eps=eps)
    hit = torch.tensor([6, 6 + T, 6 + 2 * T], device=DEV)
    assert_bits(strided[hit].view(torch.int32), can[torch.tensor([5, 5, 5], device=DEV)].view(torch.int32), "ln_stats_canonical_rows, stride 197")
    rest = torch.ones(3 * T, dtype=torch.bool, device=DEV)
    rest[hit] = False
    assert bool((strided[rest].view(torch.int32) == SENT32).all()), "strided statistics wrote other rows"
    # ---- against float64
    mean_ref, var_ref = stats_ref(X)
    d_mean, d_var = canonical_bounds(X, e32)
    mean, rstd = can[:, 0].double(), can[:, 1].double()
    var = rstd**-2 - e32
    for name in FAMILIES:
        r = fam[name]
        rm = float(((mean - mean_ref).abs()[r] / d_mean[r].clamp_min(1e-300)).max())
        rv = float(((var - var_ref).abs()[r] / d_var[r]).max())
        print(f"statistics d {d} eps {eps:g} family {name}: max err / bound: mean {rm:.3g} var {rv:.3g}")
    assert bool(((mean - mean_ref).abs() <= d_mean).all()), "canonical mean outside its bound"
    assert bool(((var - var_ref).abs() <= d_var).all()), "canonical variance outside its bound"
    # constant rows: exact sums, var == 0, rstd == float32(1 / sqrt(eps)) bit for bit
    rc = fam["constant"]
    assert torch.equal(can[rc, 0].double(), mean_ref[rc]), "constant rows: mean not exact"
    want_rstd = np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))
    assert bool((can[rc, 1].view(torch.int32) == int(np.array(want_rstd).view(np.int32))).all()), "constant rows: rstd != float32(1 / sqrt(eps))"
    # mutant: rstd from Q / d without - mean^2
    ro = fam["offset30"]
    mut_var = (X.double() ** 2).mean(1)
    assert bool((((mut_var - var_ref).abs() > 4 * d_var)[ro]).all()), "mutant 'rstd without - mean^2' is not separated on the offset rows"


def two_pass_bounds(X, eps):
    x = X.double()
    d = x.shape[1]
    e = d * 2.0**-23
    mean, var = stats_ref(X)
    sa = x.abs().sum(1)
    return e * sa / d, e * var + (e * sa / d) ** 2 + 2.0**-22 * (var + eps)


def test_two_pass_statistics_and_layernorm_rows(eng):
    d, eps = 768, 1e-12
    e32 = f32_eps(eps)
    X, fam = ln_rows(d, 777)
    rows = NP
    mean_ref, var_ref = stats_ref(X)
    d_mean, d_var = two_pass_bounds(X, e32)
    st = run_stats(eng, "ln_stats", rows, x=X, rows=rows, eps=eps)
    mean, var = st[:, 0].double(), st[:, 1].double() ** -2 - e32
    assert bool(torch.isfinite(st).all())
    print(f"ln_stats_rows: max err / bound: mean {float(((mean - mean_ref).abs() / d_mean.clamp_min(1e-300)).max()):.3g} "
          f"var {float(((var - var_ref).abs() / d_var).max()):.3g}")
    assert bool(((mean - mean_ref).abs() <= d_mean).all()), "ln_stats_rows: mean outside its bound"
    assert bool(((var - var_ref).abs() <= d_var).all()), "ln_stats_rows: variance outside its bound"
    ro = fam["offset30"]
    assert bool(((((X.double() ** 2).mean(1) - var_ref).abs() > 4 * d_var)[ro]).all()), "mutant 'rstd without - mean^2' is not separated"
    # layernorm_rows
    g = _gen(31)
    gamma, beta = (1.0 + _randn((d,), g, 0.2)).contiguous(), _randn((d,), g, 0.5)
    y = Guard(BF16, rows, d)
    eng.rowop_apply("layernorm", x=X, y=y.view, gamma=gamma, beta=beta, rows=rows, eps=eps)
    y.check("layernorm_rows")
    x = X.double()
    rstd_ref = (var_ref + e32) ** -0.5
    ref = (x - mean_ref[:, None]) * rstd_ref[:, None] * gamma.double() + beta.double()
    e = d * 2.0**-23
    tol = ulp_bf16(ref) / 2 + e * ((x.abs() + mean_ref.abs()[:, None]) * rstd_ref[:, None] * gamma.double().abs() + beta.double().abs())
    assert_close(y.valid.double(), ref, tol, "layernorm_rows")
    # mutants: beta dropped; gamma of the neighbouring column
    assert_mutant_far(ref - beta.double(), ref, tol, ref.numel() // 4, "beta dropped")
    keep = torch.cat([fam["normal"], fam["small"], fam["massive"]])
    mg = (x - mean_ref[:, None]) * rstd_ref[:, None] * torch.roll(gamma, 1).double() + beta.double()
    assert_mutant_far(mg[keep], ref[keep], tol[keep], keep.numel() * d // 8, "gamma of the neighbouring column")


@pytest.mark.parametrize("d,N", [(768, 2304), (1280, 3840)])
def test_folded_layernorm_composition(eng, d, N):
    """canonical statistics -> epilogue 5 on W' = bf16(W gamma) against f64 LayerNorm(x) . W'^T + b' (tolerance: module docstring (d))"""
    eps = 1e-12
    e32 = f32_eps(eps)
    X, fam = ln_rows(d, 99 + d)
    sel = torch.cat([fam["normal"], fam["offset30"], fam["massive"]])  # 120 rows
    M = 384  # one interior 256-row tile and a ragged one
    idx = sel[torch.arange(M, device=DEV) % sel.numel()]
    Xr = X[idx].contiguous()
    g = _gen(1234 + d)
    Wf = torch.randn((N, d), generator=g, device=DEV, dtype=F64) * 0.05
    gamma = 1.0 + 0.2 * torch.randn((d,), generator=g, device=DEV, dtype=F64)
    beta = 0.5 * torch.randn((d,), generator=g, device=DEV, dtype=F64)
    b = torch.randn((N,), generator=g, device=DEV, dtype=F64)
    Wp = (Wf * gamma).to(BF16)
    colsum = Wp.double().sum(1).float()
    bp = (b + Wf @ beta).float()
    stats = run_stats(eng, "ln_stats_canonical", M, x=Xr, row0=0, row1=M, d=d, eps=eps)
    x = Xr.double()
    mean_ref, var_ref = stats_ref(Xr)
    rstd_ref = (var_ref + e32) ** -0.5
    ref = ((x - mean_ref[:, None]) * rstd_ref[:, None]) @ Wp.double().T + bp.double()
    d_mean, d_var = canonical_bounds(Xr, e32)
    rel_rstd = d_var / (2 * (var_ref + e32)) + U
    tol = (ulp_bf16(ref) / 2 + rstd_ref[:, None] * d * 2.0**-23 * absacc64(Xr, Wp) + (d_mean * rstd_ref)[:, None] * colsum.double().abs()[None, :]
           + rel_rstd[:, None] * (ref - bp.double()).abs())
    outs = []
    for variant in (1, 3, 4):
        w = f"folded LayerNorm d {d} variant {variant}"
        out, _, _ = launch(eng, 5, Xr, Wp, variant, bias=bp, ln_stats=stats.contiguous(), colsum=colsum, what=w)
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16))
    # mutant: colsum ignored -- on the offset rows
    off = (idx >= 40) & (idx < 80)
    mut = (x * rstd_ref[:, None]) @ Wp.double().T + bp.double()
    assert_mutant_far(mut[off], ref[off], tol[off], int(off.sum()) * N // 2, "colsum ignored")


# ---------------------------------------------------------------------------------------------------------------------
# (e) row kernels


@pytest.mark.parametrize("B", [1, 3, 4, 5, 1000])
def test_cls_rows_bit_for_bit(eng, B):
    g = _gen(60 + B)
    cls, pos = _randn((768,), g), _randn((T, 768), g)
    x = Guard(BF16, B * T, 768)
    eng.rowop_apply("cls_rows", x=x.view, cls=cls, pos=pos, B=B)
    x.check("cls_rows")
    want = torch.full((B * T, 768), SENT16, dtype=torch.int16, device=DEV)
    want[torch.arange(B, device=DEV) * T] = (cls + pos[0]).to(BF16).view(torch.int16)  # one f32 addition (IEEE), then RNE
    assert_bits(x.valid_bits(), want, f"cls_rows B {B}")
    mut = want.clone()
    mut[torch.arange(B, device=DEV) * T] = (cls + pos[1]).to(BF16).view(torch.int16)
    assert_mutant_bits(mut, want, B * 384, "pos[1] for pos[0]")


def pool_ref(x, gamma, beta, eps, dtype):
    """numpy restatement of the definition in `dtype`: LayerNorm of the row, then x / max(||x||, 1e-12)"""
    x, gamma, beta = x.astype(dtype), gamma.astype(dtype), beta.astype(dtype)
    mean = x.mean(1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(1, keepdims=True, dtype=dtype)
    y = (x - mean) / np.sqrt(var + dtype(eps)) * gamma + beta
    nrm = np.sqrt((y * y).sum(1, keepdims=True, dtype=dtype))
    return y / np.maximum(nrm, dtype(1e-12))


@pytest.mark.parametrize("tok", [0, 77, 196])
def test_pool_ln_l2(eng, tok):
    B, d, eps = 37, 768, 1e-12
    rng = np.random.default_rng(500 + tok)
    xh = rng.standard_normal((B * T, d)).astype(np.float32)
    xh[(np.arange(B) * T + tok)[5]] += 30.0
    xh[(np.arange(B) * T + tok)[6]] *= 100.0
    xh[(np.arange(B) * T + tok)[7]] = 0.0  # zero row: beta / ||beta||
    gamma = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(d)).astype(np.float32)
    X = torch.from_numpy(xh).to(DEV).to(BF16)
    gm, bt = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    e32, e16 = Guard(F32, B, d), Guard(BF16, B, d)
    eng.rowop_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, B=B, tok=tok, eps=eps, emb_f32=e32.view, emb_bf16=e16.view)
    e32.check("pool_ln_l2 f32")
    e16.check("pool_ln_l2 bf16")
    got = e32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(e16.valid_bits(), got.to(BF16).view(torch.int16), "pool_ln_l2: bf16 output vs RNE of the f32 output")
    rows = X.view(B, T, d)[:, tok].float().cpu().numpy()
    ref = pool_ref(rows, gamma, beta, float(np.float32(eps)), np.float64)
    yard = float(np.abs(pool_ref(rows, gamma, beta, float(np.float32(eps)), np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print(f"pool_ln_l2 tok {tok}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, f"pool_ln_l2 tok {tok}: max deviation {err:.3g} > {tol:.3g} (float32 yardstick {yard:.3g})"
    bn = beta.astype(np.float64) / np.linalg.norm(beta.astype(np.float64))
    assert float(np.abs(got[7].double().cpu().numpy() - bn).max()) <= tol, "zero row: output is not beta / ||beta||"
    # mutants: the neighbouring token pooled; the L2 normalisation taken before beta
    other = X.view(B, T, d)[:, tok - 1 if tok else 1].float().cpu().numpy()
    assert int((np.abs(pool_ref(other, gamma, beta, eps, np.float64) - ref) > 4 * tol).sum()) >= B * d // 2, "mutant 'neighbouring token' not separated"
    # only one output requested
    only = Guard(BF16, B, d)
    eng.rowop_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, B=B, tok=tok, eps=eps, emb_bf16=only.view)
    assert torch.equal(only.valid_bits(), e16.valid_bits())


# ---------------------------------------------------------------------------------------------------------------------
# (g) argument validation: MME_E_ARG with its message, nothing launched


def test_gemm_apply_refuses_bad_arguments(eng):
    from multimodal_embeddings_amd._lib import MmeError

    M, N, K = 392, 768, 128
    g = _gen(1)
    A, W = _randn((M + 1, K), g, 1.0, BF16), _randn((N + 1, K), g, 1.0, BF16)
    bias, colsum = torch.zeros(N + 4, dtype=F32, device=DEV), torch.zeros(N + 4, dtype=F32, device=DEV)
    pos = torch.zeros((T, N), dtype=F32, device=DEV)
    stats = torch.zeros((M + 1, 2), dtype=F32, device=DEV)
    out, outf = Guard(BF16, M // NP * T, N, ld=N + 8), Guard(F32, M, N, ld=N + 4)
    res = torch.zeros((M // NP * T + 1, N + 8), dtype=BF16, device=DEV)
    planes = Guard(F32, 1, 2 * (N // 64) * 400, guard=64)
    flat16 = out.raw.view(BF16)

    def base(epi, **over):
        kw = dict(M=M, N=N, K=K, variant=3, bias=bias[:N], out=out.view, ldo=out.ld, res=res[: M // NP * T], pos=pos, outf=outf.view, ldf=outf.ld,
                  ln_stats=stats[:M], colsum=colsum[:N], ln_part=planes.view, ln_part_rows=400)
        kw.update(over)
        a, w = kw.pop("A", A[:M]), kw.pop("W", W[:N])
        return lambda: eng.gemm_apply(epi, a, w, **kw)

    bad = [
        (base(7), "epilogue 7"),
        (base(9), "outside 0..6, 8"),
        (base(0, variant=7), "variant"),
        (base(0, reverse_m=2), "reverse_m"),
        (base(0, M=0), "M ="),
        (base(0, N=0), "M ="),
        (base(0, K=96), "multiple of 64"),
        (base(0, K=0), "multiple of 64"),
        (base(0, A=None), "null operand"),
        (base(0, A=A.view(-1)[4 : 4 + M * K].view(M, K)), "16-byte aligned"),
        (base(0, W=W.view(-1)[4 : 4 + N * K].view(N, K)), "16-byte aligned"),
        (base(0, N=766), "N % 4"),
        (base(0, bias=None), "needs bias and out"),
        (base(1, out=None), "needs bias and out"),
        (base(0, bias=bias[1 : N + 1]), "bias and out must be 16-byte aligned"),
        (base(0, out=flat16[4:]), "bias and out must be 16-byte aligned"),
        (base(0, ldo=N - 8), "ldo"),
        (base(0, ldo=N + 4), "ldo"),
        (base(2, res=None), "needs res"),
        (base(2, res=res.view(-1)[4:]), "res must be 16-byte aligned"),
        (base(8, res=flat16[out.g * out.ld + 64 :]), "not overlap"),
        (base(3, M=391), "M % 196"),
        (base(3, pos=None), "needs pos"),
        (base(3, pos=pos.view(-1)[1:]), "pos must be 16-byte aligned"),
        (base(3, pos=pos[:T - 1]), "pos must hold"),
        (base(3, ln_part_rows=2 * T - 1), "ln_part_rows"),
        (base(4, outf=None), "needs outf"),
        (base(4, ldf=N - 1), "ldf"),
        (base(4, outf=outf.raw.view(F32)[1:]), "outf must be 16-byte aligned"),
        (base(5, ln_stats=None), "needs ln_stats and colsum"),
        (base(6, colsum=None), "needs ln_stats and colsum"),
        (base(5, ln_stats=stats.view(-1)[1:]), "ln_stats must be 8-byte"),
        (base(5, colsum=colsum[1 : N + 1]), "colsum 16-byte"),
        (base(8, ln_part=None), "needs ln_part"),
        (base(8, N=260, W=W[:260], bias=bias[:260]), "N % 64"),
        (base(8, ln_part_rows=M - 1), "ln_part_rows"),
        (base(8, ln_part_rows=401), "ln_part holds"),
    ]
    for call, msg in bad:
        with pytest.raises(MmeError) as ei:
            call()
        assert "(-1)" in str(ei.value) and msg in str(ei.value), f"expected MME_E_ARG with '{msg}', got: {ei.value}"
        assert out.untouched() and outf.untouched() and planes.untouched(), f"a refused call ('{msg}') wrote to its output"
    # the same arguments without the fault are accepted (the refusals above are not artefacts of the set-up)
    for epi in (0, 1, 2, 3, 4, 5, 6, 8):
        base(epi)()


def test_rowop_apply_refuses_bad_arguments(eng):
    from multimodal_embeddings_amd._lib import MmeError

    d, rows = 768, 8
    X = torch.zeros((rows * T + 1, d), dtype=BF16, device=DEV)
    vec = torch.zeros(d + 4, dtype=F32, device=DEV)
    y, st, e32 = Guard(BF16, rows, d), Guard(F32, rows * T, 2), Guard(F32, rows, d)
    part = torch.zeros(2 * 12 * 64, dtype=F32, device=DEV)
    ok = dict(x=X, y=y.view, gamma=vec[:d], beta=vec[:d], stats=st.view, part=part, cls=vec[:d], pos=vec[:d], emb_f32=e32.view, rows=rows, row0=0, row1=rows,
              stride=1, part_rows=64, d=d, B=rows, tok=0)

    def call(op, **over):
        kw = dict(ok)
        kw.update(over)
        return lambda: eng.rowop_apply(op, **kw)

    bad = [
        (call(6), "op 6 outside"),
        (call("layernorm", d=1280), "d == 768"),
        (call("ln_stats", d=704), "d == 768"),
        (call("cls_rows", d=64), "d == 768"),
        (call("pool_ln_l2", d=1280), "d == 768"),
        (call("ln_stats_canonical", d=100), "d % 64"),
        (call("ln_stats_canonical", d=2112), "d <= 2048"),
        (call("ln_finish", d=0), "d % 64"),
        (call("layernorm", x=None), "op 0 needs"),
        (call("layernorm", y=None), "op 0 needs"),
        (call("layernorm", gamma=vec[1 : d + 1]), "op 0 needs"),
        (call("layernorm", rows=-1), "rows >= 0"),
        (call("ln_stats", stats=None), "op 1 needs"),
        (call("ln_stats", x=X.view(-1)[4:]), "op 1 needs"),
        (call("ln_stats_canonical", stats=st.raw.view(F32)[1:]), "op 2 needs"),
        (call("ln_stats_canonical", row0=5, row1=4), "row0 <= row1"),
        (call("ln_stats_canonical", stride=0), "stride >= 1"),
        (call("ln_stats_canonical", row0=-1), "row0 <= row1"),
        (call("ln_finish", part=None), "op 3 needs"),
        (call("ln_finish", rows=65), "rows <= part_rows"),
        (call("ln_finish", part_rows=65, rows=8), "part_floats"),
        (call("cls_rows", cls=None), "op 4 needs"),
        (call("cls_rows", pos=vec[1 : d + 1]), "op 4 needs"),
        (call("cls_rows", B=-1), "B >= 0"),
        (call("pool_ln_l2", emb_f32=None), "emb_f32 or emb_bf16"),
        (call("pool_ln_l2", tok=197), "tok"),
        (call("pool_ln_l2", tok=-1), "tok"),
        (call("pool_ln_l2", emb_f32=e32.raw.view(F32)[1:]), "16-byte aligned"),
    ]
    for fn, msg in bad:
        with pytest.raises(MmeError) as ei:
            fn()
        assert "(-1)" in str(ei.value) and msg in str(ei.value), f"expected MME_E_ARG with '{msg}', got: {ei.value}"
        assert y.untouched() and st.untouched() and e32.untouched(), f"a refused call ('{msg}') wrote to its output"
    for op in ("layernorm", "ln_stats", "ln_stats_canonical", "ln_finish", "pool_ln_l2"):
        call(op)()
    call("cls_rows", x=torch.zeros((rows * T, d), dtype=BF16, device=DEV))()
