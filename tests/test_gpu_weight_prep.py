"""The prepared weight buffers -- what every forward starts from -- against float64 written from the MODEL's definition
(Hugging Face ViT: y = W LayerNorm(x) + b, softmax(q k / sqrt(dh)); Mllama vision: tanh-gated tables and branches), never
from the loader: the three preparation kernels one launch at a time (mme_weight_prep_apply), then every buffer of a load
read back (mme_weights_read) from both preparers, and the fingerprint kernel against its written definition.

All reference arithmetic is numpy / torch float64.  bf16 rounding is integer code written here (`bf16_rne`, checked on the
CPU against torch's own conversion); nothing comes from weights.py's rounding helpers or from csrc/.  Outputs of an apply
launch sit between sentinel guards (tests/test_gpu_gemm.py `Guard`).  The tests without the `gpu` mark run the references
against each other and assert the mutants' separation without a device.

(a) One launch at a time.
    convert  all 65536 bf16 patterns, all 65536 f16 patterns, and for f32 all 65536 high halves under each of six low
             halves (ties, their neighbours, the round-up into the next binade and into infinity); unscaled, times
             f32(0.125 log2 e) and times 2^-120 (normals into f32 subnormals); to an f32 table and to bf16.  Bit for bit
             against the numpy f32 product followed by one RNE rounding; a NaN must leave as a NaN with the quiet bit set
             (payload free); zeros, subnormals and infinities bit-exact.  Mutants: truncation for RNE (wherever a rounding
             happens: not bf16 -> bf16 unscaled, where the conversion is the identity), flush of subnormal inputs (unscaled
             and log2 e runs), flush of subnormal products (2^-120 runs, where a flushed input gives the same zero).
             One f32 -> bf16 launch of 2048 * 256 * 8 + 24 elements (one chunk past a single sweep of the largest grid)
             with hashed values; count 8; count 0.
    pad      (rows, cols, cols_padded) = (1, 4, 4), (3, 4, 8), (1280, 588, 640), (4100, 588, 640: past 2048 * 256 quads,
             the stride loop), (5, 588, 592), three dtypes; bit for bit, pad columns +0.0.  Mutants: source pitch
             cols_padded (where rows > 1 and cols_padded > cols), pad columns unwritten (where cols_padded > cols).
    fold     five cases up to three sources, every dtype, K 64 .. 1280.  Inputs representable in the case's dtype (the f32
             cases keep 11 significant bits) so that w * gamma of an unscaled row is exact in f32 (asserted); planted at
             gamma = 1: -0.0, a subnormal, 1e38 (6e4 in f16), the bf16 tie 1 + 2^-8 (f32, f16), and in every dtype the tie
             3 (1 + 2^-7) as a PRODUCT; beta carries a subnormal and a -0.0.
             W' unscaled rows: bits of the f64 product rounded once.  W' scaled rows: |W' - s w gamma| <= ulp_bf16/2 +
             2^-22 |s w gamma| (rounding of s, of s w and of (s w) gamma in f32: 3 x 2^-24).  colsum against the EXACT sum
             of the returned W' (f64 sum where every partial sum is representable, math.fsum on the other rows) within
             ulp_f32/2 + K 2^-53 sum |W'|.  b' against b_eff + sum_k w_eff beta_k in f64 within ulp_f32/2 + (K + 2) 2^-53
             (|b_eff| + sum |w_eff beta|), scaled rows + 2^-23 of the same magnitude.
             Mutants: colsum of the unrounded products; b' from W'; gamma and beta exchanged; the scale on source 1; the
             scale left off source 0's bias; source 1 read from row 0 of source 0.  K walked DESCENDING is not separated
             by these bounds (the f64 sums differ by parts in 2^53, the outputs are f32): its figures are printed, nothing
             is asserted.
    refusals one call per precondition: MME_E_ARG, guarded outputs untouched.
(b) Every buffer of a load, from the device preparer (a checkpoint directory) and the host preparer (the same values as
    f32): ViT 384 / 6 heads / 2 layers / mlp 128 in bf16, ViT 1024 / 16 / 1 / 64 in f16, the shallow tower (2 local + 1
    global) in bf16; LayerNorm gamma = 1 + 0.25 z, beta = 0.25 z; tower gates 0.7, 0.3, -0.4 (tables), 0.5, -0.8 (global layer).
    The table (index, name, definition) follows include/mme.h; 6 + 18 L and 11 + 9 L buffers, counted.
    Plain f32 tables: identical bits.  Plain bf16: one RNE.  qkv_w / qkv_b: Q rows under the scaled-row bound (f32 half
    ulp for qkv_b), K | V bit for bit.  Folded triples as in (a).  Tower tables with a factor f (tanh g, or 1 - tanh g):
    the library takes tanh in f32 from libm (1 ulp allowed), 1 - g and the product in f32, so with d_f = ulp_f32(tanh g)
    (+ ulp_f32(1 - tanh g) / 2 for pos):  |got - f x| <= ulp_f32(f x)/2 + d_f |x|, and + ulp_bf16(f x)/2 for the bf16
    matrices o_w / fc2_w of the global layer.  Local layers untouched, zeros zero, patch_w padded.
    Mutants (reference side): layernorm_before / _after exchanged, K / V exchanged, the scale without log2 e, dh = 64 in
    the tower, tanh left off the gates, pos / tilepos factors exchanged, a gate on a local layer, gate_attn / gate_ffn
    exchanged.
    Function: per folded triple, 64 rows x (mean offsets 0, 3, 30):  r (W' x - mu colsum) + b'  against
    W_eff (gamma (x - mu) r + beta) + b_eff  within  r 2^-9 sum_k |w_eff gamma| |x_k - mu| + |mu r| ulp_f32(colsum)/2 +
    ulp_f32(b')/2: the fold MEANS LayerNorm followed by the linear map.
    Fingerprint: word i == sum(word * odd_hash(word index)) mod 2^64 over the read-back bytes (numpy uint64, odd_hash
    from include/mme.h); the two preparers' buffers are byte-equal; two words exchanged change the reference word.

Recorded.  On an MI355X: NOT YET -- no device run of this file has been made; every bounded case prints its `max err / tol`
and every table mutant its count (`pytest -s`), to be copied here.  Without a device (the two tests at the end): the
numpy product + integer RNE equal torch's arithmetic and conversion on all 391682 / 65282 / 63490 non-NaN patterns (f32 /
bf16 / f16) under each of the three scales; the fold reference's f64 sum of w beta is within 0.0017 of K 2^-53 sum|w beta|
of math.fsum and the f64 colsum of bf16 values equals math.fsum on every row; every mutant is separated (table mutants:
K / V exchanged 294634 .. 294668 of 442368 elements and 768 of 1152; LayerNorms exchanged 437930 of 442368 and 24469 of
24576; no log2 e 147455 of 442368 and 384 of 1152; the tower's eight between 1638378 of 4915200 (dh 64: the Q third) and
all but a few zeros of a table); K descending: 0 colsums differ in bits in every case.  A numpy emulation of the library's
arithmetic (f32 scale, f32 product, RNE, f64 sums one k after the other) passes every fold check with max err / tol 0.98
.. 1.00 (a correctly rounded result reaches the half-ulp bounds) and the function check at 0.14 .. 0.31 of its bound.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_gemm import BF16, DEV, F32, F64, SENT16, Guard, assert_bits, assert_close, assert_mutant_bits, assert_mutant_far, ulp_bf16

gpu = pytest.mark.gpu
F16 = torch.float16
DT_TORCH = {0: F32, 1: BF16, 2: F16}
DT_ID = {"float32": 0, "bfloat16": 1, "float16": 2}
LOG2E = 1.4426950408889634  # log2(e), float64
I16, I32, I64 = torch.int16, torch.int32, torch.int64


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# number formats, written here


def bf16_rne(x32):
    """f32 tensor -> bf16 bits (int16), round to nearest even in integer arithmetic; a NaN keeps its top bits and gets the
    quiet bit"""
    u = x32.contiguous().view(I32).to(I64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = torch.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, r) & 0xFFFF
    return (r - ((r & 0x8000) << 1)).to(I16)


def bf16_bits_to_f64(b):
    return ((b.to(I32) & 0xFFFF) << 16).view(F32).double()


def ulp_f32(x):
    """spacing of f32 at |x| (f64 in, f64 out); the subnormal spacing at and near 0"""
    _, e = torch.frexp(x.abs())
    u = torch.ldexp(torch.ones_like(x), e - 24).clamp_min(2.0**-149)
    return torch.where(x == 0, torch.full_like(x, 2.0**-149), u)


def exact_f32(x64, what):
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), f"{what}: a value the reference rounds once is not exact in f32"
    return x32


def exact_rowsum(v):
    """correctly rounded exact row sums of f64 [R, K] holding bf16 values.  A bf16 value m 2^e (frexp) is a multiple of
    2^(e - 8); with e_min, e_max over a row's non-zero entries every partial sum is a multiple of 2^(e_min - 8) below
    K 2^e_max, so the f64 sum is exact in any order when e_max - e_min + 8 + log2 K <= 53.  Other rows: math.fsum."""
    s = v.sum(1)
    a = v.abs()
    _, e = torch.frexp(a)
    big = torch.full_like(e, 1 << 20)
    emin = torch.where(a > 0, e, big).min(1).values
    emax = torch.where(a > 0, e, -big).max(1).values
    unsafe = (emax - emin + 8 + math.ceil(math.log2(v.shape[1])) > 53) & (emax > -(1 << 20))
    for r in unsafe.nonzero().reshape(-1).tolist():
        s[r] = math.fsum(v[r].tolist())
    return s


def count_far(a, ref, tol):
    return int(((a - ref).abs() > 4 * tol).sum())


# ---------------------------------------------------------------------------------------------------------------------
# (a) convert

LOWS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
S_Q = np.float32(0.125 * LOG2E)
S_SUB = np.float32(2.0**-120)
SCALES = {"unscaled": None, "log2e/8": S_Q, "2^-120": S_SUB}
SWEEP = 2048 * 256 * 8  # elements the largest grid covers in one sweep


def convert_inputs(dt):
    """(the stored bit patterns, their values widened to f32 -- exact for all three types)"""
    if dt == 0:
        hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
        bits = np.concatenate([hi | np.uint32(lo) for lo in LOWS])
        return bits, bits.view(np.float32)
    bits = np.arange(65536, dtype=np.uint16)
    if dt == 1:
        return bits, (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits, bits.view(np.float16).astype(np.float32)


def subnormal_inputs(dt, x32):
    """inputs that are subnormal in their OWN type"""
    a = np.abs(x32)
    return (a > 0) & (a < (2.0**-14 if dt == 2 else 2.0**-126))


def convert_ref(x32, scale, out_bf16, truncate=False, flush_in=None, flush_out=False):
    """-> (bits as uint32 / uint16, NaN mask): the numpy f32 product, then one RNE rounding"""
    x = x32.copy()
    if flush_in is not None:
        x[flush_in] = np.copysign(np.float32(0), x[flush_in])
    with np.errstate(all="ignore"):
        y = (x * scale if scale is not None else x).astype(np.float32)
    if flush_out:
        sub = (np.abs(y) > 0) & (np.abs(y) < 2.0**-126)
        y[sub] = np.copysign(np.float32(0), y[sub])
    nan = np.isnan(y)
    u = y.view(np.uint32)
    if not out_bf16:
        return u.copy(), nan
    if truncate:
        return (u >> np.uint32(16)).astype(np.uint16), nan
    return bf16_rne(torch.from_numpy(y)).numpy().view(np.uint16).copy(), nan


def convert_mutants(dt, x32, scale, out_bf16):
    """[(name, bits, least)] for one run; `least` elements must differ from the reference in bits"""
    name = [k for k, v in SCALES.items() if v is scale][0]
    out = []
    if out_bf16 and not (dt == 1 and scale is None):
        out.append(("truncation for RNE", convert_ref(x32, scale, True, truncate=True)[0], 1000))
    if name == "2^-120":
        out.append(("subnormal products flushed to zero", convert_ref(x32, scale, out_bf16, flush_out=True)[0], 1000))
    else:
        out.append(("subnormal inputs flushed to zero", convert_ref(x32, scale, out_bf16, flush_in=subnormal_inputs(dt, x32))[0], 100))
    return out


def check_convert(got, want, nan, out_bf16, what):
    qbit, mag, inf = (0x0040, 0x7FFF, 0x7F80) if out_bf16 else (0x00400000, 0x7FFFFFFF, 0x7F800000)
    g = got.astype(np.int64)
    g_nan = (g & mag) > inf
    assert np.array_equal(g_nan, nan), f"{what}: {int((g_nan != nan).sum())} elements are NaN on one side only"
    assert bool(((g[nan] & qbit) != 0).all()), f"{what}: {int(((g[nan] & qbit) == 0).sum())} NaNs left without the quiet bit"
    assert_bits(torch.from_numpy(np.where(nan, 0, g)).reshape(-1, 8), torch.from_numpy(np.where(nan, 0, want.astype(np.int64))).reshape(-1, 8), what)


def run_convert(eng, dt, bits, scale, out_bf16, what, count=None):
    n = bits.size if count is None else count
    src = torch.from_numpy(bits.view(np.int32 if dt == 0 else np.int16)).to(DEV)
    out = Guard(BF16 if out_bf16 else F32, 1, max(n, 8), guard=1)
    eng.weight_prep_apply("convert", dtype=dt, src=src, dst=out.view, count=n, scale=1.0 if scale is None else float(scale), scaled=scale is not None,
                          out_bf16=out_bf16)
    out.check(what)
    return out, out.valid_bits().reshape(-1).cpu().numpy().view(np.uint16 if out_bf16 else np.uint32)


def assert_convert_mutants(dt, x32, scale, out_bf16, want, nan, what):
    for name, bits, least in convert_mutants(dt, x32, scale, out_bf16):
        assert_mutant_bits(torch.from_numpy(np.where(nan, 0, bits.astype(np.int64))), torch.from_numpy(np.where(nan, 0, want.astype(np.int64))), least,
                           f"{what}: {name}")


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_convert_dense_bit_patterns(eng, dt):
    bits, x32 = convert_inputs(dt)
    for sname, scale in SCALES.items():
        for out_bf16 in (False, True):
            what = f"convert {('f32', 'bf16', 'f16')[dt]} -> {'bf16' if out_bf16 else 'f32'} {sname}"
            want, nan = convert_ref(x32, scale, out_bf16)
            assert_convert_mutants(dt, x32, scale, out_bf16, want, nan, what)
            _, got = run_convert(eng, dt, bits, scale, out_bf16, what)
            check_convert(got, want, nan, out_bf16, what)
            print(f"{what}: {got.size} patterns equal in bits, {int(nan.sum())} NaNs quiet")


def stride_inputs():
    n = SWEEP + 24
    i = np.arange(n, dtype=np.uint64)
    bits = ((i * np.uint64(2654435761)) & np.uint64(0xBFFFFFFF)).astype(np.uint32)  # exponent below 2^1: finite, a value per index
    return bits, bits.view(np.float32)


@gpu
def test_convert_grid_stride_loop(eng):
    bits, x32 = stride_inputs()
    want, nan = convert_ref(x32, None, True)
    assert not nan.any() and not (want == SENT16).any()
    unwritten = want.copy()
    unwritten[SWEEP:] = SENT16
    assert_mutant_bits(torch.from_numpy(unwritten.astype(np.int64)), torch.from_numpy(want.astype(np.int64)), 24, "elements beyond the first sweep unwritten")
    out, got = run_convert(eng, 0, bits, None, True, "stride loop")
    assert not (got == SENT16).any(), f"{int((got == SENT16).sum())} elements of the valid range keep the guard pattern (first at {int(np.argmax(got == SENT16))})"
    check_convert(got, want, nan, True, f"convert f32 -> bf16, {bits.size} elements")
    out8, got8 = run_convert(eng, 0, bits[:8], None, True, "count 8")
    check_convert(got8, want[:8], nan[:8], True, "convert count 8")
    out0, _ = run_convert(eng, 0, bits[:8], None, True, "count 0", count=0)
    assert out0.untouched(), "count 0 wrote to its output"


# ---------------------------------------------------------------------------------------------------------------------
# (a) pad

PAD_SHAPES = [(1, 4, 4), (3, 4, 8), (1280, 588, 640), (4100, 588, 640), (5, 588, 592)]


def pad_inputs(dt, rows, cols, dev):
    g = torch.Generator().manual_seed(rows * 1000 + cols + dt)
    x = (torch.randn((rows, cols), generator=g) * 0.05).to(DT_TORCH[dt])
    x[0, 1], x[rows - 1, cols - 1], x[0, 2], x[rows // 2, 0] = -0.0, 1.0 + 2.0**-8, 1e-39 if dt != 2 else 6e-8, 1e38 if dt != 2 else 6e4
    return x.to(dev)


def pad_ref(x, cp, pitch=None, pad_bits=0):
    rows, cols = x.shape
    src = x
    if pitch is not None:  # the source walked with another row pitch (indices wrap: a reference-side mutant reads nothing out of bounds)
        idx = (torch.arange(rows, device=x.device)[:, None] * pitch + torch.arange(cols, device=x.device)[None, :]) % x.numel()
        src = x.reshape(-1)[idx]
    out = torch.full((rows, cp), pad_bits, dtype=I16, device=x.device)
    out[:, :cols] = bf16_rne(src.float())
    return out


def pad_mutants(x, cp, want):
    rows, cols = x.shape
    if rows > 1 and cp > cols:
        assert_mutant_bits(pad_ref(x, cp, pitch=cp), want, rows * cols // 4, "source rows walked with pitch cols_padded")
    if cp > cols:
        assert_mutant_bits(pad_ref(x, cp, pad_bits=SENT16), want, rows * (cp - cols), "pad columns left unwritten")


@gpu
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", PAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pad(eng, dt, shape):
    rows, cols, cp = shape
    x = pad_inputs(dt, rows, cols, DEV)
    want = pad_ref(x, cp)
    pad_mutants(x, cp, want)
    out = Guard(BF16, rows, cp, ld=cp, guard=4)
    eng.weight_prep_apply("pad", dtype=dt, src=x, dst=out.view, rows=rows, cols=cols, cols_padded=cp)
    out.check(f"pad {shape}")
    assert_bits(out.valid_bits(), want, f"pad {shape} dtype {dt}")


# ---------------------------------------------------------------------------------------------------------------------
# (a) fold: the reference, shared with (b)


def fold_ref(Ws, bs, scales, gamma, beta):
    """The fold of LayerNorm (gamma, beta) into y = W x + b from its definition, float64.  Ws: f64 [rows_i, K]; bs: f64
    [rows_i] or None; scales: the TRUE scale of a source (float64) or None.  p = s w gamma; t = sum_k s w beta_k."""
    p, scaled, beff, t, tabs = [], [], [], [], []
    for W, b, s in zip(Ws, bs, scales):
        sw = W if s is None else W * s
        p.append(sw * gamma)
        terms = sw * beta
        t.append(terms.sum(1))
        tabs.append(terms.abs().sum(1))
        b = torch.zeros(W.shape[0], dtype=F64, device=W.device) if b is None else b
        beff.append(b if s is None else b * s)
        scaled.append(torch.full((W.shape[0],), s is not None, device=W.device))
    c = torch.cat
    return dict(p=c(p), scaled=c(scaled), beff=c(beff), t=c(t), tabs=c(tabs), K=Ws[0].shape[1])


def fold_tols(ref, wf):
    """(cs_ref, cs_tol, bf_ref, bf_tol, w_tol) for returned W' values wf (f64)"""
    K, sc = ref["K"], ref["scaled"].double()
    cs_ref = exact_rowsum(wf)
    cs_tol = ulp_f32(cs_ref) / 2 + K * 2.0**-53 * wf.abs().sum(1)
    bf_ref = ref["beff"] + ref["t"]
    mag = ref["beff"].abs() + ref["tabs"]
    bf_tol = ulp_f32(bf_ref) / 2 + (K + 2) * 2.0**-53 * mag + sc * 2.0**-23 * mag
    w_tol = ulp_bf16(ref["p"]) / 2 + 2.0**-22 * ref["p"].abs()
    return cs_ref, cs_tol, bf_ref, bf_tol, w_tol


def fold_assert(out, ref, what):
    """out = (W' bits int16 [R, K], colsum f64 [R], b' f64 [R]) as the library returned them"""
    bits, cs, bf = out
    wf = bf16_bits_to_f64(bits)
    cs_ref, cs_tol, bf_ref, bf_tol, w_tol = fold_tols(ref, wf)
    un = ~ref["scaled"]
    if un.any():
        assert_bits(bits[un], bf16_rne(exact_f32(ref["p"][un], what)), f"{what}: W' unscaled rows")
    if ref["scaled"].any():
        sc = ref["scaled"]
        assert_close(wf[sc], ref["p"][sc], w_tol[sc], f"{what}: W' scaled rows")
    assert_close(cs[None], cs_ref[None], cs_tol[None], f"{what}: colsum")
    assert_close(bf[None], bf_ref[None], bf_tol[None], f"{what}: b'")


def fold_emulate(ref, cs=None, bf=None):
    """what a kernel computing `ref`'s definition returns, up to its own rounding: W' = bf16(p), colsum = its exact sum"""
    bits = bf16_rne(ref["p"].float())
    return bits, (exact_rowsum(bf16_bits_to_f64(bits)) if cs is None else cs), (ref["beff"] + ref["t"] if bf is None else bf)


def fold_caught(out, ref):
    """elements of a (mutant) output triple that fold_assert's rule rejects with margin: bits on the unscaled W' rows, 4 x the
    tolerance elsewhere -> (W', colsum, b')"""
    bits, cs, bf = out
    wf = bf16_bits_to_f64(bits)
    cs_ref, cs_tol, bf_ref, bf_tol, w_tol = fold_tols(ref, wf)
    un, sc = ~ref["scaled"], ref["scaled"]
    nw = int((bits[un] != bf16_rne(ref["p"][un].float())).sum()) + count_far(wf[sc], ref["p"][sc], w_tol[sc])
    return nw, count_far(cs, cs_ref, cs_tol), count_far(bf, bf_ref, bf_tol)


def assert_fold_mutant(name, out, ref, channel, least):
    n = fold_caught(out, ref)["W' colsum b'".split().index(channel)]
    assert n >= least, f"mutant '{name}' is rejected on {n} elements of {channel} only (< {least}): the case would not catch it"


FOLD_CASES = [  # (dtype, rows per source, cols, source 0 scaled, source 1 without bias)
    (0, [64], 64, False, False),
    (1, [128, 64], 384, True, True),
    (2, [64, 64, 64], 1280, True, False),
    (1, [384, 384, 384], 384, True, False),
    (0, [256], 1024, False, False),
]


def fold_inputs(case, dev):
    dt, rows, K, scaled0, null_b1 = case
    tdt = DT_TORCH[dt]
    g = torch.Generator().manual_seed(1000 * K + sum(rows) + dt)

    def rep(x):  # representable in the case's dtype; the f32 cases keep f16's 11 bits, so that w * gamma is exact in f32
        return (x.to(F16) if dt == 0 else x).to(tdt)

    big, sub = (6e4, 6e-8) if dt == 2 else (1e38, 1e-39)
    gamma, beta = rep(1 + 0.25 * torch.randn(K, generator=g)), rep(0.25 * torch.randn(K, generator=g))
    gamma[5], gamma[6] = 1.0, 1.0 + 2.0**-7
    beta[9], beta[11] = sub, -0.0
    Ws, bs = [], []
    for i, r in enumerate(rows):
        W = rep(0.05 * torch.randn((r, K), generator=g))
        for j, row in enumerate((0, 31, r - 1)):
            W[row, 5] = (1.0 + 2.0**-8, big, sub)[j]  # under gamma = 1 (the tie is not a bf16 value: that case has the product tie only)
            W[row, 6] = 3.0                           # 3 (1 + 2^-7): a bf16 tie as a product
            W[row, 9] = -0.0
        Ws.append(W.to(dev))
        bs.append(None if (null_b1 and i == 1) else rep(0.1 * torch.randn(r, generator=g)).to(dev))
    scales = [0.125 * LOG2E if (scaled0 and i == 0) else None for i in range(len(rows))]
    return dict(dt=dt, rows=rows, K=K, Ws=Ws, bs=bs, scales=scales, gamma=gamma.to(dev), beta=beta.to(dev))


def fold_ref_of(c, Ws=None, bs=None, scales=None, gamma=None, beta=None):
    d = lambda t: None if t is None else t.double()  # noqa: E731
    return fold_ref([d(w) for w in (Ws or c["Ws"])], [d(b) for b in (bs or c["bs"])], scales or c["scales"], d(c["gamma"] if gamma is None else gamma),
                    d(c["beta"] if beta is None else beta))


def sequential_sums(v, descending):
    """f64 row sums of v [R, K] (numpy) taken one k after the other"""
    s = np.zeros(v.shape[0])
    for k in (range(v.shape[1] - 1, -1, -1) if descending else range(v.shape[1])):
        s = s + v[:, k]
    return s


def fold_mutants(c, ref, what):
    """asserts the separation of every mutant of the case; -> the figures of the unseparated one (K descending)"""
    rows, R = c["rows"], sum(c["rows"])
    true = fold_emulate(ref)
    assert fold_caught(true, ref) == (0, 0, 0), f"{what}: the reference does not pass its own check"
    wq = bf16_bits_to_f64(true[0])
    assert_fold_mutant("colsum of the unrounded w * gamma", fold_emulate(ref, cs=ref["p"].sum(1)), ref, "colsum", R // 2)
    beta = c["beta"].double()
    assert_fold_mutant("b' summed with W' in place of w", fold_emulate(ref, bf=ref["beff"] + (wq * beta).sum(1)), ref, "b'", R // 2)
    assert_fold_mutant("gamma and beta exchanged", fold_emulate(fold_ref_of(c, gamma=c["beta"], beta=c["gamma"])), ref, "W'", R * c["K"] // 2)
    r0 = rows[0]
    if len(rows) > 1 and c["scales"][0] is not None:
        swapped = [c["scales"][1], c["scales"][0]] + c["scales"][2:]
        assert_fold_mutant("the scale applied to source 1", fold_emulate(fold_ref_of(c, scales=swapped)), ref, "W'", (r0 + rows[1]) * c["K"] // 2)
    if c["scales"][0] is not None:
        bf = (ref["beff"] + ref["t"]).clone()
        bf[:r0] = c["bs"][0].double() + ref["t"][:r0]
        assert_fold_mutant("the scale left off the bias of source 0", fold_emulate(ref, bf=bf), ref, "b'", r0 // 2)
    if len(rows) > 1:
        Ws = [c["Ws"][0], c["Ws"][0][: rows[1]]] + c["Ws"][2:]
        assert_fold_mutant("source 1 read from row 0 of source 0", fold_emulate(fold_ref_of(c, Ws=Ws)), ref, "W'", rows[1] * c["K"] // 2)
    # K descending: the same f64 terms in the other order, rounded to f32 once
    wq_np = wq.cpu().numpy()
    asc, desc = sequential_sums(wq_np, False), sequential_sums(wq_np, True)
    differ = int((asc.astype(np.float32) != desc.astype(np.float32)).sum())
    cs_tol = fold_tols(ref, wq)[1].cpu().numpy()
    print(f"{what}: K descending (NOT separated, not asserted): {differ} of {R} f32 colsums differ in bits; max |asc - desc| / tol = "
          f"{float((np.abs(asc - desc) / cs_tol).max()):.3g}")
    return differ


def run_fold(eng, c, what):
    R, K = sum(c["rows"]), c["K"]
    wf, cs, bf = Guard(BF16, R, K), Guard(F32, 1, R, guard=1), Guard(F32, 1, R, guard=1)
    eng.weight_prep_apply("fold", dtype=c["dt"], w=c["Ws"], b=c["bs"], src_rows=c["rows"], cols=K, gamma=c["gamma"], beta=c["beta"], wf=wf.view, cs=cs.view,
                          bf=bf.view, src_scale=[1.0 if s is None else float(np.float32(s)) for s in c["scales"]], src_scaled=[s is not None for s in c["scales"]])
    for gd in (wf, cs, bf):
        gd.check(what)
    return wf.valid_bits(), cs.valid.reshape(-1).double(), bf.valid.reshape(-1).double()


def _case_id(c):
    return f"{('f32', 'bf16', 'f16')[c[0]]}-{'+'.join(map(str, c[1]))}x{c[2]}"


@gpu
@pytest.mark.parametrize("case", FOLD_CASES, ids=_case_id)
def test_fold(eng, case):
    what = "fold " + _case_id(case)
    c = fold_inputs(case, DEV)
    ref = fold_ref_of(c)
    fold_mutants(c, ref, what)
    fold_assert(run_fold(eng, c, what), ref, what)


# ---------------------------------------------------------------------------------------------------------------------
# (a) refusals


@gpu
def test_weight_prep_apply_refuses_bad_arguments(eng):
    from multimodal_embeddings_amd._lib import MmeError

    src32 = torch.zeros(64 * 64 + 8, dtype=F32, device=DEV)
    src16 = torch.zeros(64 * 64 + 8, dtype=BF16, device=DEV)
    vec = torch.zeros(64 + 8, dtype=F32, device=DEV)
    o32, o16 = Guard(F32, 1, 64, guard=1), Guard(BF16, 8, 8, guard=4)
    wf, cs, bf = Guard(BF16, 64, 64), Guard(F32, 1, 64, guard=1), Guard(F32, 1, 64, guard=1)
    outs = (o32, o16, wf, cs, bf)
    W, g = src32[: 64 * 64], vec[:64]
    ok = {
        "convert": dict(dtype=0, src=src32[:64], dst=o32.view, count=64),
        "pad": dict(dtype=1, src=src16[:32], dst=o16.view, rows=8, cols=4, cols_padded=8),
        "fold": dict(dtype=0, w=[W], b=[g], src_rows=[64], cols=64, gamma=g, beta=g, wf=wf.view, cs=cs.view, bf=bf.view),
    }

    def call(op, **over):
        kw = dict(ok.get(op, ok["convert"]))
        kw.update(over)
        return lambda: eng.weight_prep_apply(op, **kw)

    raw32, raw16 = o32.raw.view(F32), o16.raw.view(BF16)
    bad = [
        (call(3), "op 3 outside"),
        (call(-1), "op -1 outside"),
        (call("convert", dtype=3), "dtype 3"),
        (call("pad", dtype=-1), "dtype -1"),
        (call("fold", dtype=7), "dtype 7"),
        (call("convert", count=12), "count % 8 == 0"),
        (call("convert", count=-8), "0 <= count"),
        (call("convert", count=2**40 + 8), "count <= 2^40"),
        (call("convert", src=None), "op 0 needs src, dst non-null"),
        (call("convert", dst=None), "op 0 needs src, dst non-null"),
        (call("convert", src=src32[1:65]), "16-byte aligned"),
        (call("convert", dst=raw32[65:]), "16-byte aligned"),
        (call("convert", dtype=1, src=src16[4:68]), "16-byte aligned"),
        (call("pad", rows=0), "rows >= 1"),
        (call("pad", cols=0), "cols >= 4"),
        (call("pad", cols=6, cols_padded=8), "cols % 4 == 0"),
        (call("pad", cols_padded=10), "cols_padded % 4 == 0"),
        (call("pad", cols=8, cols_padded=4), "cols_padded >= cols"),
        (call("pad", src=None), "op 1 needs src, dst non-null"),
        (call("pad", dst=None), "op 1 needs src, dst non-null"),
        (call("pad", src=src16[4:36]), "16-byte aligned"),
        (call("pad", dst=raw16[36:]), "16-byte aligned"),
        (call("fold", nsrc=0), "nsrc in 1..3"),
        (call("fold", nsrc=4), "nsrc in 1..3"),
        (call("fold", cols=0), "cols a multiple of 64"),
        (call("fold", cols=96), "cols a multiple of 64"),
        (call("fold", cols=1344), "cols <= 1280"),
        (call("fold", src_rows=[0]), "non-zero multiple of 64"),
        (call("fold", src_rows=[32]), "non-zero multiple of 64"),
        (call("fold", src_rows=[2**24 + 64]), "<= 2^24"),
        (call("fold", w=[W, W], src_rows=[64, 96]), "non-zero multiple of 64"),
        (call("fold", w=[None], nsrc=1), "every w[i] non-null"),
        (call("fold", w=[W, None], src_rows=[64, 64]), "every w[i] non-null"),
        (call("fold", w=[src32[1 : 64 * 64 + 1]]), "every w[i] non-null and 16-byte aligned"),
        (call("fold", dtype=1, w=[src16[: 64 * 64]], b=[src32.view(torch.uint8)[1:129]], gamma=src16[:64], beta=src16[:64]), "every b[i] null or aligned"),
        (call("fold", gamma=None), "gamma, beta, wf, cs, bf non-null"),
        (call("fold", beta=None), "gamma, beta, wf, cs, bf non-null"),
        (call("fold", gamma=vec[1:65]), "gamma, beta, wf, cs, bf non-null and 16-byte aligned"),
        (call("fold", beta=vec[2:66]), "gamma, beta, wf, cs, bf non-null and 16-byte aligned"),
        (call("fold", wf=None), "gamma, beta, wf, cs, bf non-null"),
        (call("fold", cs=None), "gamma, beta, wf, cs, bf non-null"),
        (call("fold", bf=None), "gamma, beta, wf, cs, bf non-null"),
        (call("fold", cs=cs.raw.view(F32)[65:]), "gamma, beta, wf, cs, bf non-null and 16-byte aligned"),
        (call("fold", wf=wf.raw.view(BF16)[3 * 64 + 4 :]), "gamma, beta, wf, cs, bf non-null and 16-byte aligned"),
    ]
    for fn, msg in bad:
        with pytest.raises(MmeError) as ei:
            fn()
        assert "(-1)" in str(ei.value) and msg in str(ei.value), f"expected MME_E_ARG with '{msg}', got: {ei.value}"
        assert all(o.untouched() for o in outs), f"a refused call ('{msg}') wrote to its output"
    # the same arguments without the fault are accepted (the refusals above are not artefacts of the set-up); a null bias is one of them
    for op in ok:
        call(op)()
    call("fold", b=[None])()


# ---------------------------------------------------------------------------------------------------------------------
# (b) every prepared buffer of a load

SEED = 7
GATES = {"pos": 0.7, "pre": 0.3, "post": -0.4, "attn": 0.5, "ffn": -0.8}


def _spread_layernorms(w, specs, seed):
    """every LayerNorm gamma <- 1 + 0.25 z, beta <- 0.25 z (seeded), so that the LayerNorms of a layer are far apart"""
    from multimodal_embeddings_amd.weights import irwin_hall_normal

    for tid, spec in enumerate(specs):
        name, shape = spec[0], spec[1]
        if "layernorm" in name or "layer_norm" in name:
            z = irwin_hall_normal(seed + 100, tid, int(np.prod(shape))).reshape(shape) * np.float32(0.25)
            w[name] = (z + np.float32(1.0) if name.endswith(".weight") else z).astype(np.float32)
    return w


def vit_weights(geom):
    from multimodal_embeddings_amd.weights import make_vit_weights, vit_tensor_specs

    return _spread_layernorms(make_vit_weights(SEED, geom), vit_tensor_specs(geom), SEED)


def tower_weights(geom):
    from multimodal_embeddings_amd.weights import make_tile_vit_weights, tile_vit_tensor_specs

    w = _spread_layernorms(make_tile_vit_weights(SEED, geom), tile_vit_tensor_specs(geom), SEED)
    w["gated_positional_embedding.gate"][:] = GATES["pos"]
    w["pre_tile_positional_embedding.gate"][:] = GATES["pre"]
    w["post_tile_positional_embedding.gate"][:] = GATES["post"]
    for i in range(geom.num_global_layers):
        w[f"global_transformer.layers.{i}.gate_attn"][:] = GATES["attn"]
        w[f"global_transformer.layers.{i}.gate_ffn"][:] = GATES["ffn"]
    return w


class Factor:
    """a factor the library forms in f32: its true value (float64) and the bound of the f32 factor's error"""

    def __init__(self, value, err):
        self.value, self.err = value, err


def _ulp32(v):
    return float(ulp_f32(torch.tensor([v], dtype=F64))[0])


def gate_factors(gate, tanh=True):
    """(tanh g, 1 - tanh g) as Factors: tanh from libm in f32 within 1 ulp; 1 - g adds the half ulp of its own rounding"""
    t = math.tanh(gate) if tanh else gate
    return Factor(t, _ulp32(t)), Factor(1.0 - t, _ulp32(t) + _ulp32(1.0 - t) / 2)


# A table is a list of (name, kind, definition), one entry per prepared buffer in the order include/mme.h documents.
#   "f32"   identical bits of the tensor          "bf16"  one RNE rounding of the tensor
#   "f32*"  (tensor, Factor) f32 table            "bf16*" (tensor, Factor) bf16 matrix
#   "zeros" n f32 zeros                           "pad"   (tensor [rows, cols], cols_padded)
#   "qkv_w" / "qkv_b"  a fold definition: Q | K | V concatenated, the Q part times the scale
#   "fold"  a fold definition: the W' of a triple; "cs" / "bf": the colsum and b' that belong to the W' before them
# A fold definition is dict(W=[..], b=[..], s=[..], gamma, beta, eps).


def vit_table(m, g, mut=None):
    D, F = g.hidden_size, g.intermediate_size
    s = g.head_dim**-0.5 * (1.0 if mut == "scale without log2(e)" else LOG2E)
    t = [("cls", "f32", m["embeddings.cls_token"]), ("pos", "f32", m["embeddings.position_embeddings"]),
         ("patch_b", "f32", m["embeddings.patch_embeddings.projection.bias"]), ("lnf_g", "f32", m["layernorm.weight"]), ("lnf_b", "f32", m["layernorm.bias"]),
         ("patch_w", "bf16", m["embeddings.patch_embeddings.projection.weight"])]
    for l in range(g.num_layers):
        p = f"layers.{l}."
        ln1, ln2 = ("layernorm_after", "layernorm_before") if mut == "layernorm_before and _after exchanged" else ("layernorm_before", "layernorm_after")
        q, k, v = ("q_proj", "v_proj", "k_proj") if mut == "K and V exchanged" else ("q_proj", "k_proj", "v_proj")
        qkv = dict(W=[m[p + f"attention.{n}.weight"] for n in (q, k, v)], b=[m[p + f"attention.{n}.bias"] for n in (q, k, v)], s=[s, None, None],
                   gamma=m[p + ln1 + ".weight"], beta=m[p + ln1 + ".bias"], eps=g.layer_norm_eps)
        fc1 = dict(W=[m[p + "mlp.fc1.weight"]], b=[m[p + "mlp.fc1.bias"]], s=[None], gamma=m[p + ln2 + ".weight"], beta=m[p + ln2 + ".bias"],
                   eps=g.layer_norm_eps)
        t += [(f"{l}.ln1_g", "f32", m[p + "layernorm_before.weight"]), (f"{l}.ln1_b", "f32", m[p + "layernorm_before.bias"]),
              (f"{l}.ln2_g", "f32", m[p + "layernorm_after.weight"]), (f"{l}.ln2_b", "f32", m[p + "layernorm_after.bias"]),
              (f"{l}.qkv_w", "qkv_w", qkv), (f"{l}.qkv_b", "qkv_b", qkv), (f"{l}.qkv_wf", "fold", qkv), (f"{l}.qkv_cs", "cs", qkv), (f"{l}.qkv_bf", "bf", qkv),
              (f"{l}.o_w", "bf16", m[p + "attention.o_proj.weight"]), (f"{l}.o_b", "f32", m[p + "attention.o_proj.bias"]),
              (f"{l}.fc1_w", "bf16", m[p + "mlp.fc1.weight"]), (f"{l}.fc1_b", "f32", m[p + "mlp.fc1.bias"]),
              (f"{l}.fc1_wf", "fold", fc1), (f"{l}.fc1_cs", "cs", fc1), (f"{l}.fc1_bf", "bf", fc1),
              (f"{l}.fc2_w", "bf16", m[p + "mlp.fc2.weight"]), (f"{l}.fc2_b", "f32", m[p + "mlp.fc2.bias"])]
    assert len(t) == 6 + 18 * g.num_layers
    return t


def tower_table(m, g, mut=None):
    D, F = g.hidden_size, g.intermediate_size
    gate = lambda name: float(m[name].double().reshape(-1)[0])  # noqa: E731
    th = mut != "tanh left off the gates"
    s = (64 if mut == "dh = 64 for the tower" else g.head_dim) ** -0.5 * LOG2E
    f_tile, f_pos = gate_factors(gate("gated_positional_embedding.gate"), th)
    if mut == "pos and tilepos factors exchanged":
        f_tile, f_pos = f_pos, f_tile
    f_pre, f_post = gate_factors(gate("pre_tile_positional_embedding.gate"), th)[0], gate_factors(gate("post_tile_positional_embedding.gate"), th)[0]
    t = [("cls", "f32", m["class_embedding"]), ("pos", "f32*", (m["gated_positional_embedding.embedding"], f_pos)),
         ("tilepos", "f32*", (m["gated_positional_embedding.tile_embedding.weight"], f_tile)),
         ("pre", "f32*", (m["pre_tile_positional_embedding.embedding.weight"], f_pre)),
         ("post", "f32*", (m["post_tile_positional_embedding.embedding.weight"], f_post)),
         ("lnpre_g", "f32", m["layernorm_pre.weight"]), ("lnpre_b", "f32", m["layernorm_pre.bias"]),
         ("lnpost_g", "f32", m["layernorm_post.weight"]), ("lnpost_b", "f32", m["layernorm_post.bias"]),
         ("zeros", "zeros", F), ("patch_w", "pad", (m["patch_embedding.weight"].reshape(D, -1), 640))]
    g0 = "global_transformer.layers.0."
    for l in range(g.num_layers + g.num_global_layers):
        gated = l >= g.num_layers
        p = f"global_transformer.layers.{l - g.num_layers}." if gated else f"transformer.layers.{l}."
        fa = ff = None
        if gated or (mut == "a gate applied to a local layer" and l == 0):
            src = p if gated else g0
            fa, ff = gate_factors(gate(src + "gate_attn"), th)[0], gate_factors(gate(src + "gate_ffn"), th)[0]
            if mut == "gate_attn and gate_ffn exchanged":
                fa, ff = ff, fa
        qkv = dict(W=[m[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], b=[None] * 3, s=[s, None, None], gamma=m[p + "input_layernorm.weight"],
                   beta=m[p + "input_layernorm.bias"], eps=g.norm_eps)
        fc1 = dict(W=[m[p + "mlp.fc1.weight"]], b=[m[p + "mlp.fc1.bias"]], s=[None], gamma=m[p + "post_attention_layernorm.weight"],
                   beta=m[p + "post_attention_layernorm.bias"], eps=g.norm_eps)
        gated_or = lambda kind, x, f: (kind, x) if f is None else (kind + "*", (x, f))  # noqa: E731
        t += [(f"{l}.qkv_wf", "fold", qkv), (f"{l}.qkv_cs", "cs", qkv), (f"{l}.qkv_bf", "bf", qkv),
              (f"{l}.o_w",) + gated_or("bf16", m[p + "self_attn.o_proj.weight"], fa),
              (f"{l}.fc1_wf", "fold", fc1), (f"{l}.fc1_cs", "cs", fc1), (f"{l}.fc1_bf", "bf", fc1),
              (f"{l}.fc2_w",) + gated_or("bf16", m[p + "mlp.fc2.weight"], ff), (f"{l}.fc2_b",) + gated_or("f32", m[p + "mlp.fc2.bias"], ff)]
    assert len(t) == 11 + 9 * (g.num_layers + g.num_global_layers)
    return t


def fold_ref_of_def(d):
    dd = lambda t: None if t is None else t.double()  # noqa: E731
    return fold_ref([dd(w) for w in d["W"]], [dd(b) for b in d["b"]], d["s"], dd(d["gamma"]), dd(d["beta"]))


def expectation(kind, d):
    """-> ("bf16" | "f32", [(lo, hi, "bits", bits) | (lo, hi, "close", ref, tol)]) over the flat elements of a plain buffer"""
    if kind in ("f32", "bf16"):
        x = exact_f32(d.double().reshape(-1), kind)
        return kind, [(0, x.numel(), "bits", x.view(I32) if kind == "f32" else bf16_rne(x))]
    if kind in ("f32*", "bf16*"):
        x, f = d[0].double().reshape(-1), d[1]
        ref = x * f.value
        tol = ulp_f32(ref) / 2 + f.err * x.abs() + (ulp_bf16(ref) / 2 if kind == "bf16*" else 0)
        return kind[:-1], [(0, x.numel(), "close", ref, tol)]
    if kind == "zeros":
        return "f32", [(0, d, "bits", torch.zeros(d, dtype=I32, device=DEV_OF[0]))]
    if kind == "pad":
        return "bf16", [(0, d[0].shape[0] * d[1], "bits", pad_ref(d[0].float(), d[1]).reshape(-1))]
    if kind in ("qkv_w", "qkv_b"):
        x = [(w if kind == "qkv_w" else b).double().reshape(-1) for w, b in zip(d["W"], d["b"])]
        n, ref = x[0].numel(), x[0] * d["s"][0]
        rest = exact_f32(torch.cat(x[1:]), kind)
        if kind == "qkv_w":
            return "bf16", [(0, n, "close", ref, ulp_bf16(ref) / 2 + 2.0**-22 * ref.abs()), (n, 3 * n, "bits", bf16_rne(rest))]
        return "f32", [(0, n, "close", ref, ulp_f32(ref) / 2 + 2.0**-22 * ref.abs()), (n, 3 * n, "bits", rest.view(I32))]
    raise AssertionError(kind)


DEV_OF = ["cpu"]  # where the model tensors of the table being evaluated live


def decode(raw, fmt):
    """read-back bytes (uint8 tensor) -> (bits, f64 values)"""
    if fmt == "bf16":
        bits = raw.view(I16)
        return bits, bf16_bits_to_f64(bits)
    bits = raw.view(I32)
    return bits, bits.view(F32).double()


def check_plain(name, kind, d, raw):
    fmt, parts = expectation(kind, d)
    bits, val = decode(raw, fmt)
    assert bits.numel() == parts[-1][1], f"{name}: {bits.numel()} elements read back, {parts[-1][1]} expected"
    for part in parts:
        lo, hi = part[0], part[1]
        if part[2] == "bits":
            assert_bits(bits[lo:hi].reshape(1, -1), part[3].reshape(1, -1), f"{name} [{lo}, {hi})")
        else:
            assert_close(val[lo:hi].reshape(1, -1), part[3].reshape(1, -1), part[4].reshape(1, -1), f"{name} [{lo}, {hi})")


def plain_mutant_count(kind, d_true, d_mut):
    """elements on which the mutant's definition leaves the true one: other bits, or beyond 4 x the tolerance"""
    n = 0
    kind_m, d_m = d_mut
    (_, pt), (_, pm) = expectation(kind, d_true), expectation(kind_m, d_m)
    if [p[2] for p in pt] != [p[2] for p in pm]:  # an exact buffer became a scaled one (or the reverse): compare as values
        fmt = expectation(kind, d_true)[0]
        val = lambda p: (bf16_bits_to_f64(p[3]) if fmt == "bf16" else p[3].view(F32).double()) if p[2] == "bits" else p[3]  # noqa: E731
        tol = lambda p: (ulp_bf16(val(p)) / 2 if fmt == "bf16" else ulp_f32(val(p)) / 2) if p[2] == "bits" else p[4]  # noqa: E731
        return sum(count_far(val(b), val(a), tol(a)) for a, b in zip(pt, pm))
    for a, b in zip(pt, pm):
        n += int((a[3] != b[3]).sum()) if a[2] == "bits" else count_far(b[3], a[3], a[4])
    return n


def check_table(table, bufs, what):
    """every buffer of a load against its definition; -> {name of a fold's W': (definition, (bits, cs, bf))}"""
    assert len(bufs) == len(table), f"{what}: {len(bufs)} prepared buffers, the table has {len(table)}"
    folds = {}
    for i, (name, kind, d) in enumerate(table):
        if kind in ("cs", "bf"):
            continue
        raw = torch.from_numpy(bufs[i]).to(DEV_OF[0])
        if kind != "fold":
            check_plain(f"{what} [{i}] {name}", kind, d, raw)
            continue
        assert table[i + 1][1] == "cs" and table[i + 2][1] == "bf"
        ref = fold_ref_of_def(d)
        R, K = ref["p"].shape
        assert bufs[i].size == R * K * 2 and bufs[i + 1].size == R * 4 and bufs[i + 2].size == R * 4, f"{what} [{i}] {name}: sizes of the triple"
        out = (raw.view(I16).reshape(R, K), decode(torch.from_numpy(bufs[i + 1]).to(DEV_OF[0]), "f32")[1], decode(torch.from_numpy(bufs[i + 2]).to(DEV_OF[0]), "f32")[1])
        fold_assert(out, ref, f"{what} [{i}] {name}")
        folds[name] = (d, out)
    return folds


def check_table_mutants(build, m, g, mutants, what):
    """each mutant of the definitions leaves the true table, on the named buffers, by the project's rule"""
    true = {name: (kind, d) for name, kind, d in build(m, g)}
    for mut, names in mutants.items():
        mt = {name: (kind, d) for name, kind, d in build(m, g, mut)}
        for name in names:
            kind, d = true[name]
            if kind == "fold":
                ref = fold_ref_of_def(d)
                n, total = fold_caught(fold_emulate(fold_ref_of_def(mt[name][1])), ref)[0], ref["p"].numel()
                least = total // 4  # a third of a Q | K | V matrix, at least
            else:
                n, total = plain_mutant_count(kind, d, mt[name]), expectation(kind, d)[1][-1][1]
                least = total // 4
            print(f"{what}: mutant '{mut}' leaves {name} on {n} of {total} elements")
            assert n >= least, f"mutant '{mut}' is rejected on {n} of {total} elements of {name} only (< {least}): the table would not catch it"


VIT_MUTANTS = {
    "layernorm_before and _after exchanged": ["0.qkv_wf", "0.fc1_wf"],
    "K and V exchanged": ["0.qkv_w", "0.qkv_b", "0.qkv_wf"],
    "scale without log2(e)": ["0.qkv_w", "0.qkv_b", "0.qkv_wf"],
}
TOWER_MUTANTS = {
    "dh = 64 for the tower": ["0.qkv_wf", "2.qkv_wf"],
    "tanh left off the gates": ["pos", "tilepos", "pre", "post", "2.o_w", "2.fc2_w", "2.fc2_b"],
    "pos and tilepos factors exchanged": ["pos", "tilepos"],
    "a gate applied to a local layer": ["0.o_w", "0.fc2_w", "0.fc2_b"],
    "gate_attn and gate_ffn exchanged": ["2.o_w", "2.fc2_w", "2.fc2_b"],
}


def function_check(name, d, out, seed, what):
    """r (W' x - mu colsum) + b' against W_eff (gamma (x - mu) r + beta) + b_eff on 64 rows x with mean offsets 0, 3, 30"""
    bits, cs, bf = out
    dev = bits.device
    dd = lambda t: t.double()  # noqa: E731
    W = torch.cat([dd(w) * (1.0 if s is None else s) for w, s in zip(d["W"], d["s"])])
    b = torch.cat([torch.zeros(w.shape[0], dtype=F64, device=dev) if bb is None else dd(bb) * (1.0 if s is None else s) for w, bb, s in zip(d["W"], d["b"], d["s"])])
    gamma, beta, K = dd(d["gamma"]), dd(d["beta"]), W.shape[1]
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((64, K), generator=g, dtype=F64) + torch.tensor([0.0, 3.0, 30.0], dtype=F64).repeat_interleave(22)[:64, None]).to(dev)
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    r = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + d["eps"])
    wq = bf16_bits_to_f64(bits)
    left = r * (x @ wq.T - mu * cs[None]) + bf[None]
    right = (gamma * xc * r + beta) @ W.T + b[None]
    tol = r * 2.0**-9 * (xc.abs() @ (W * gamma).abs().T) + (mu * r).abs() * ulp_f32(cs)[None] / 2 + ulp_f32(bf)[None] / 2
    assert_close(left, right, tol, f"{what} {name}: LayerNorm then the linear map")
    return left, right, tol, (x, xc, r, W, b)


class Load:
    """one geometry loaded by both preparers: the model tensors (checkpoint dtype, on the device), the read-back buffers"""


def _read_all(e):
    fp = e.weights_fingerprint()
    return [e.weights_read(i) for i in range(len(fp))], fp


def _load_vit(tmp, geom, dtype):
    from multimodal_embeddings_amd import checkpoint as ckpt
    from multimodal_embeddings_amd._lib import Engine

    ckpt.save_checkpoint(tmp, vit_weights(geom), "vit", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp, "vit")
    assert ck.dtype == dtype and ck.geometry == geom
    L = Load()
    L.geom, L.build, L.mutants = geom, vit_table, VIT_MUTANTS
    L.m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_vit_checkpoint(ck)
        host.load_vit({k: t.float().numpy() for k, t in ck.tensors.items()}, eps=geom.layer_norm_eps)
        (L.dev, L.fp_dev), (L.host, L.fp_host) = _read_all(dev), _read_all(host)
    finally:
        dev.close()
        host.close()
    return L


def _load_tower(tmp):
    from multimodal_embeddings_amd import checkpoint as ckpt
    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import TileViTGeometry

    geom = TileViTGeometry(num_layers=2, num_global_layers=1, intermediate_layers=(0,))
    ckpt.save_checkpoint(tmp, tower_weights(geom), "mllama_tiles", "bfloat16", geom)
    ck = ckpt.read_checkpoint(tmp, "mllama_tiles")
    assert ck.dtype == "bfloat16" and ck.geometry == geom
    L = Load()
    L.geom, L.build, L.mutants = geom, tower_table, TOWER_MUTANTS
    L.m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_tile_vit_checkpoint(ck)
        host.load_tile_vit({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (L.dev, L.fp_dev), (L.host, L.fp_host) = _read_all(dev), _read_all(host)
    finally:
        dev.close()
        host.close()
    return L


@pytest.fixture(scope="module")
def loads(tmp_path_factory):
    from multimodal_embeddings_amd.weights import ViTGeometry

    cache = {}

    def get(key):
        if key not in cache:
            tmp = tmp_path_factory.mktemp(key)
            if key == "vit384-bf16":
                cache[key] = _load_vit(tmp, ViTGeometry(hidden_size=384, num_layers=2, num_heads=6, intermediate_size=128), "bfloat16")
            elif key == "vit1024-f16":
                cache[key] = _load_vit(tmp, ViTGeometry(hidden_size=1024, num_layers=1, num_heads=16, intermediate_size=64), "float16")
            else:
                cache[key] = _load_tower(tmp)
        return cache[key]

    return get


LOADS = ["vit384-bf16", "vit1024-f16", "tower-bf16"]


@gpu
@pytest.mark.parametrize("key", LOADS)
def test_every_prepared_buffer(loads, key):
    L = loads(key)
    DEV_OF[0] = DEV
    table = L.build(L.m, L.geom)
    layers = L.geom.num_layers + getattr(L.geom, "num_global_layers", 0)
    assert len(L.fp_dev) == len(L.fp_host) == len(table) == (11 + 9 * layers if key.startswith("tower") else 6 + 18 * layers)
    check_table_mutants(L.build, L.m, L.geom, L.mutants, key)
    folds = check_table(table, L.dev, f"{key} device")
    for i, (a, b) in enumerate(zip(L.dev, L.host)):
        assert a.size == b.size and np.array_equal(a, b), f"{key}: buffer [{i}] {table[i][0]} differs between the device and the host preparer"
    for k, (name, (d, out)) in enumerate(folds.items()):
        left, right, tol, (x, xc, r, W, b) = function_check(name, d, out, 100 + k, key)
        other = [dd for n, (dd, _) in folds.items() if n[:2] == name[:2] and n != name]
        if other:  # the other LayerNorm of the same layer in the definition
            gm, bt = other[0]["gamma"].double(), other[0]["beta"].double()
            assert_mutant_far((gm * xc * r + bt) @ W.T + b[None], right, tol, right.numel() // 2, f"{key} {name}: the other LayerNorm's gamma and beta")


def odd_hash(x):
    """include/mme.h: the splitmix64 finaliser, forced odd (numpy uint64, wrapping)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (x ^ (x >> np.uint64(31))) | np.uint64(1)


def fingerprint_ref(raw):
    """sum(word * odd_hash(word index)) mod 2^64 over the little-endian 32-bit words of a byte buffer; up to three bytes behind
    the last whole word count as one more word, zero-extended"""
    words = raw.size // 4
    total = np.uint64(0)
    step = 1 << 23
    with np.errstate(over="ignore"):
        for o in range(0, words, step):
            w = raw[4 * o : 4 * min(o + step, words)].view("<u4").astype(np.uint64)
            total = total + (w * odd_hash(np.arange(o, o + w.size, dtype=np.uint64))).sum(dtype=np.uint64)
        if raw.size & 3:
            tail = np.uint64(int.from_bytes(raw[4 * words :].tobytes(), "little"))
            total = total + tail * odd_hash(np.array([words], dtype=np.uint64))[0]
    return int(total)


@gpu
@pytest.mark.parametrize("key", LOADS)
def test_fingerprint_is_its_definition(loads, key):
    L = loads(key)
    for i, raw in enumerate(L.dev):
        want = fingerprint_ref(raw)
        assert L.fp_dev[i] == want, f"{key}: fingerprint word {i} is {L.fp_dev[i]:#x}, the definition gives {want:#x}"
        assert L.fp_host[i] == want, f"{key}: the host preparer's fingerprint word {i} is {L.fp_host[i]:#x}, the definition gives {want:#x}"
    # two words of a buffer exchanged change the reference word (the checksum depends on position)
    raw = L.dev[1][: 1 << 16].copy()
    w = raw.view("<u4")
    j = int(np.argmax(w != w[0]))
    assert j > 0
    before = fingerprint_ref(raw)
    w[0], w[j] = w[j], w[0]
    assert fingerprint_ref(raw) != before


@gpu
def test_weights_read_arguments():
    from multimodal_embeddings_amd._lib import Engine, MmeError

    e = Engine(0)
    try:
        with pytest.raises(MmeError, match=r"\(-1\).*index 0 outside"):
            e.weights_read(0)  # nothing loaded
        e.load_vit(vit_weights(_tiny_geom()))
        n = len(e.weights_fingerprint())
        for idx in (-1, n):
            with pytest.raises(MmeError, match=r"\(-1\).*index"):
                e.weights_read(idx)
        assert e.lib.mme_weights_read(e.h, 0, 16, None) == -1 and e.lib.mme_weights_read(e.h, 0, -1, None) == -1
        assert e.lib.mme_weights_read(e.h, 0, 0, None) == 384 * 4
        part = np.full(32, 0xA5, dtype=np.uint8)
        assert e.lib.mme_weights_read(e.h, 0, 16, part.ctypes.data) == 384 * 4  # a short capacity copies that much and no more
        assert np.array_equal(part[:16], e.weights_read(0)[:16]) and bool((part[16:] == 0xA5).all())
    finally:
        e.close()


def _tiny_geom():
    from multimodal_embeddings_amd.weights import ViTGeometry

    return ViTGeometry(hidden_size=384, num_layers=1, num_heads=6, intermediate_size=64)


# ---------------------------------------------------------------------------------------------------------------------
# without a device: the references against each other, and the separation of every mutant


def test_references_agree_without_a_device():
    """numpy against torch: the f32 product and the integer RNE code against torch's own arithmetic and conversion on every
    convert pattern; the fold reference's sums against math.fsum."""
    for dt in (0, 1, 2):
        _, x32 = convert_inputs(dt)
        for sname, scale in SCALES.items():
            want, nan = convert_ref(x32, scale, True)
            t = torch.from_numpy(x32)
            y = t * float(scale) if scale is not None else t
            assert y.dtype == F32
            tb = y.to(BF16).view(I16).numpy().view(np.uint16)
            w32, _ = convert_ref(x32, scale, False)
            assert np.array_equal(y.view(I32).numpy().view(np.uint32)[~nan], w32[~nan]), (dt, sname, "f32 product")
            assert np.array_equal(tb[~nan], want[~nan]), (dt, sname, "RNE")
            print(f"dtype {dt} {sname}: {int((~nan).sum())} products and roundings equal between numpy + integer RNE and torch")
    worst_cs = worst_bf = 0.0
    for case in FOLD_CASES:
        c = fold_inputs(case, "cpu")
        ref = fold_ref_of(c)
        wq = bf16_bits_to_f64(fold_emulate(ref)[0])
        fs = torch.tensor([math.fsum(row) for row in wq.tolist()], dtype=F64)
        assert torch.equal(exact_rowsum(wq), fs), f"{_case_id(case)}: exact_rowsum is not math.fsum"
        terms = torch.cat([(w.double() * (1.0 if s is None else s)) * c["beta"].double() for w, s in zip(c["Ws"], c["scales"])])
        ft = torch.tensor([math.fsum(row) for row in terms.tolist()], dtype=F64)
        err, bound = (ref["t"] - ft).abs(), case[2] * 2.0**-53 * ref["tabs"]
        assert bool((err <= bound).all())
        worst_bf = max(worst_bf, float((err / bound.clamp_min(1e-300)).max()))
        worst_cs = max(worst_cs, float(((wq.sum(1) - fs).abs() / (case[2] * 2.0**-53 * wq.abs().sum(1))).max()))
    print(f"fold reference: f64 sum of w beta against math.fsum, max err / (K 2^-53 sum|.|) = {worst_bf:.3g}; plain f64 colsum against math.fsum {worst_cs:.3g}")


def test_mutants_are_separated_without_a_device():
    for dt in (0, 1, 2):
        _, x32 = convert_inputs(dt)
        for sname, scale in SCALES.items():
            for out_bf16 in (False, True):
                want, nan = convert_ref(x32, scale, out_bf16)
                assert_convert_mutants(dt, x32, scale, out_bf16, want, nan, f"convert {dt} {sname} {out_bf16}")
    for shape in PAD_SHAPES:
        if shape[0] <= 1280:
            for dt in (0, 1, 2):
                x = pad_inputs(dt, shape[0], shape[1], "cpu")
                pad_mutants(x, shape[2], pad_ref(x, shape[2]))
    for case in FOLD_CASES:
        c = fold_inputs(case, "cpu")
        fold_mutants(c, fold_ref_of(c), "fold " + _case_id(case))
    geom = _tiny_geom()
    DEV_OF[0] = "cpu"
    m = {k: torch.from_numpy(v).to(BF16) for k, v in vit_weights(geom).items()}
    check_table_mutants(vit_table, m, geom, VIT_MUTANTS, "vit384-bf16 (1 layer)")
