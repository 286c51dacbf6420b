"""SigLIP ViT/16 image towers on the GPU (196 tokens, tanh-GELU, attention-pooling head): the kernels the tower adds, one
launch at a time (mme_siglip_apply, mme_attention_apply under a SigLIP context); the prepared weight buffers; the whole pass
against the float32 restatement of tests/siglip_reference.py and the rows transformers itself returned
(tests/golden/siglip_cases.npz); bit identities; coexistence with CLIP on one context; refusals.

(1) attention at T = 196 (attention.hip instantiated at 196 tokens) against the float64 pass of tests/test_gpu_attention.py's
    definition, restated here for 196 tokens, with that file's bound |got - ref| <= 2^-8 |ref| + 2^-8 A, A = sum p |v| / sum p,
    in all three attention modes (exact, fast, fast with the re-run forced).
(2) the tanh-GELU epilogues against float64.  Tolerance: half a bf16 ulp of the result (with the 2^-6 room of
    tests/test_gpu_gemm.py's gelu_tol), plus the f32 evaluation: the exponent z = x (c0 + c1 x^2) log2 e / 2 is formed with a
    relative error of a few 2^-24, which exp2 turns into a relative error of that times |z| -- 8 x 2^-24 (1 + |z|) |ref| as
    tests/test_gpu_clip.py's qgelu_tol has it for its exponent -- plus 2^-126 where the result leaves the normal range.
(3) embed_rows_t196 BIT FOR BIT: two IEEE f32 additions in a stated order and one round-to-nearest-even.
(4) map_pool against float64: |got - ref| <= 2^-8 |ref| + 2^-8 A, A = sum p |v| / sum p: the output is rounded to bf16 once
    (2^-9 |ref|), the f32 scores, exponentials and sums over 196 terms are orders below; the bound of (1) covers it with room.
(5) l2_rows_bf16 against float64 with the rule of the pool forms (8 x a float32 restatement's own deviation, at least 2^-22).
(6) end to end: max(1 - cos) <= 1e-3, the project's standing bound for the bf16 path.  Measured values: DESIGN.md 4.15.
    What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
    tests/test_gpu_tower_sharpness.py.
"""
import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_siglip_golden as mks  # noqa: E402
import siglip_reference as sr  # noqa: E402
from test_gpu_clip import _golden_crops, _pack, _uniform, l2_ref_np  # noqa: E402
from test_gpu_gemm import (BF16, DEV, F32, F64, SENT16, Guard, _gen, _randn, absacc64, acc64, assert_bits, assert_close, assert_mutant_bits,  # noqa: E402
                           assert_mutant_far, expect_256, gelu_ref, ulp_bf16)

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, SIGLIP_B16, SiglipGeometry, make_clip_weights, make_siglip_weights, round_to_bf16,  # noqa: E402
                                               synthetic_crops)

pytestmark = pytest.mark.gpu

I16, I32 = torch.int16, torch.int32
T, DH = 196, 64
LOG2E = 1.4426950408889634
CASES = mks.CASES  # B16s: 768 x 2; S16: 384 x 2, MLP 1536; L16: 1024 x 2, MLP 4096
MODES = (0, 1, 2)
_weights = {}
_fault = []


@pytest.fixture(autouse=True)
def _a_fault_ends_the_module():
    if _fault:
        pytest.fail(f"not run: an earlier test of this module met a GPU fault ({_fault[0]})")
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _fault.append(str(e)[:200])
        raise


def weights_of(key):
    if key not in _weights:
        _weights[key] = make_siglip_weights(*CASES[key])
    return _weights[key]


def tiny(H):
    return SiglipGeometry(hidden_size=64 * H, num_layers=1, num_heads=H, intermediate_size=64)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sig():
    """{heads: a context that holds a one-layer SigLIP tower of that many heads}: kind 0 of mme_attention_apply runs T = 196 there"""
    engines = {}
    for H in (6, 12, 16):
        e = Engine(0)
        e.load_siglip(make_siglip_weights(40 + H, tiny(H)), tiny(H))
        engines[H] = e
    yield engines
    for e in engines.values():
        e.close()


@pytest.fixture(scope="module")
def crops40():
    return torch.from_numpy(synthetic_crops(40, seed=3)).cuda()


def _close_all(emb):
    for e in emb.engines:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (1) attention at 196 tokens


def _random_qkv(n, H, seed, q_scale=0.25, tokens=T, extra_rows=0):
    g = _gen(seed)
    rows = n * tokens
    x = torch.empty((rows + extra_rows, 3, H * DH), dtype=BF16, device=DEV)
    x[:rows, 0] = _randn((rows, H * DH), g, q_scale, BF16)
    x[:rows, 1] = _randn((rows, H * DH), g, 1.0, BF16)
    x[:rows, 2] = _randn((rows, H * DH), g, 1.0, BF16)
    return x.view(rows + extra_rows, 3 * H * DH)


def _view(qkv, H, tokens=T):
    return qkv.view(-1, tokens, 3, H, DH)


def reference(qkv, H, mutant=None, tokens=T):
    """float64 (out, A), each [n, T, H, dh]; mutant(s [n, H, T, T]) -> scores replaces the true scores (a named kernel bug)"""
    x = _view(qkv, H, tokens).double()
    q, k, v = (x[:, :, j].permute(0, 2, 1, 3) for j in range(3))  # [n, H, T, dh]
    s = q @ k.transpose(-1, -2)
    if mutant:
        s = mutant(s)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p @ v) / l).permute(0, 2, 1, 3), ((p @ v.abs()) / l).permute(0, 2, 1, 3)


def _tol(ref, A):
    return 2.0**-8 * (ref.abs() + A)


def _same(a, b):
    return torch.equal(a.view(I16), b.view(I16))


def run_modes(e, qkv, **kw):
    """{mode: (out, redone)} with the mode-independent contract of tests/test_gpu_attention.py checked; every launch writes
    between guard rows"""
    res = {}
    n = qkv.shape[0] // T
    H = qkv.shape[1] // (3 * DH)
    try:
        for mode in MODES:
            e.set_attention_mode(mode)
            buf = Guard(BF16, n * T, H * DH)
            _, redone = e.attention(qkv, 0, out=buf.view, **kw)
            buf.check(f"attention T = 196, mode {mode}")
            res[mode] = (buf.valid.clone(), redone)
    finally:
        e.set_attention_mode(1)
    assert not res[0][1], "mode 0 reported a re-run"
    assert res[2][1], "mode 2 did not re-run"
    assert _same(res[2][0], res[0][0]), "mode 2 (forced re-run) differs from mode 0"
    if res[1][1]:
        assert _same(res[1][0], res[0][0]), "mode 1 reported a re-run but its output is not the exact kernel's"
    return res


def check_all(res, ref, A, H, what):
    for mode, (out, redone) in res.items():
        assert_close(out.view(-1, T, H, DH).double(), ref, _tol(ref, A), f"{what}, mode {mode} (redone {int(redone)})")


@pytest.mark.parametrize("H,n", [(6, 1), (6, 3), (12, 1), (12, 3), (16, 1), (16, 3), (12, 22)])
def test_attention_196_random(sig, H, n):
    """Distinct data for every (crop, head).  n = 22 at 12 heads: 264 blocks on a grid of 256 workgroups, eight of which walk on
    to a second block (the persistent stride)."""
    qkv = _random_qkv(n, H, 1000 + 7 * H + n)
    res = run_modes(sig[H], qkv)
    assert not res[1][1], "ordinary scores raised the fast form's guard"
    ref, A = reference(qkv, H)
    check_all(res, ref, A, H, f"attention T = 196 random H {H} n {n}")
    assert sig[H].encoder_info()["kind"] == "siglip"


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_196_zero_queries_average_exactly_the_196_value_rows(sig, H):
    """Q = 0: every score is 0 and the output is the mean of the crop's own 196 V rows.  LDS rows 196..199 hold clamped copies
    of row 195: counted as keys they would weigh V[195] five times; read unclamped they would be the next crop's first rows
    -- and, behind the LAST crop, the row that follows the activation: that row holds NaN here, so one read of it shows."""
    n = 2
    big = _random_qkv(n, H, 300 + H, extra_rows=1)
    big[n * T :] = float("nan")
    qkv = big[: n * T]
    assert qkv.is_contiguous() and qkv.data_ptr() == big.data_ptr()
    x = _view(qkv, H)
    x[:, :, 0] = 0.0
    x[1, 0, 2] = 100.0  # V row 0 of crop 1: what crop 0 would meet as key 196 under the 197-token stride
    ref, A = reference(qkv, H)
    mean = x[:, :, 2].double().mean(1, keepdim=True).expand(n, T, H, DH)
    assert bool(((ref - mean).abs() <= 1e-12 * A).all())  # the reference IS the mean
    res = run_modes(sig[H], qkv)
    assert not res[1][1]
    check_all(res, ref, A, H, f"attention T = 196, Q = 0, H {H}")
    tol = _tol(ref, A)
    v = x[:, :, 2].double()
    counted = ((v.sum(1, keepdim=True) + 4 * v[:, 195:196]) / 200).expand(n, T, H, DH)  # the clamped copies as keys
    assert_mutant_far(counted[0], ref[0], tol[0], T * H * DH // 4, "padding rows 196..199 counted as keys")  # (4 of 200 keys: a small shift)
    spill = ((v[0].sum(0, keepdim=True) + v[1, :1].sum(0, keepdim=True)) / 197).expand(T, H, DH)  # 197 keys: crop 1's row 0 as key 196
    assert_mutant_far(spill, ref[0], tol[0], T * H * DH // 2, "the 197-token stride: the next crop's first row as key 196")


SPIKE_KEYS = (31, 32, 191, 192, 195)
SPIKE_ROWS = [0, 31, 32, 191, 192, 195]


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_196_spikes_at_tile_and_padding_borders(sig, H):
    """Spike keys at the borders of the 32-key tiles and at the last token (whose clamped copies fill LDS rows 196..199), for
    queries at the borders of the query blocks; the spike holds most of the row's mass, so both dropping it and counting it
    five times move the output."""
    n = 3
    qkv = _random_qkv(n, H, 400 + H)
    x = _view(qkv, H)
    x[:, :, 1, :, 0] = 0.0  # dim 0 of K: zero except at the spike key
    key_of = torch.tensor([[SPIKE_KEYS[(i * H + h) % len(SPIKE_KEYS)] for h in range(H)] for i in range(n)], device=DEV)
    for i in range(n):
        for h in range(H):
            x[i, int(key_of[i, h]), 1, h, 0] = 10.0
            x[i, SPIKE_ROWS, 0, h, 0] = 1.0
    res = run_modes(sig[H], qkv)
    assert not res[1][1]
    ref, A = reference(qkv, H)
    check_all(res, ref, A, H, f"attention T = 196 spikes H {H}")
    tol = _tol(ref, A)
    onehot = torch.nn.functional.one_hot(key_of, T).bool()[:, :, None, :]  # [n, H, 1, T]

    def dropped(s):
        return s.masked_fill(onehot, float("-inf"))

    def pad_counted(s):  # keys 196..199 are copies of key 195: key 195 weighs 5 x
        s = s.clone()
        s[..., 195] += float(np.log2(5.0))
        return s

    for name, mutant in (("the spike key dropped", dropped), ("padding rows counted as keys", pad_counted)):
        mref, _ = reference(qkv, H, mutant)
        ratio = ((mref - ref).abs() / tol)[:, SPIKE_ROWS].amax(-1)  # [n, rows, H]
        sel = ratio if mutant is dropped else ratio.permute(0, 2, 1)[key_of == 195]
        assert sel.numel() and bool((sel >= 4).all()), f"mutant '{name}' is not separated: {sel.min()}"


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_196_huge_last_key_raises_the_guard(sig, H):
    """K row 195 is huge and finite (|k| = 1e30: scores of ~1e30 in either sign, finite in f32), far above the fast form's
    reference point (the maximum over key tile 0): its guard fires, the launch is redone by the exact form and the output is
    the exact form's, bit for bit.  The clamped copies of row 195 in LDS rows 196..199 are removed by selection."""
    n = 2
    qkv = _random_qkv(n, H, 500 + H)
    x = _view(qkv, H)
    x[:, 195, 1] = torch.where(x[:, 195, 1] > 0, 1e30, -1e30).to(BF16)
    ref, A = reference(qkv, H)
    assert bool(torch.isfinite(ref).all())
    res = run_modes(sig[H], qkv)
    assert res[1][1], "the fast form's guard did not fire"
    assert _same(res[1][0], res[0][0])
    check_all(res, ref, A, H, f"attention T = 196 huge key 195, H {H}")


def test_attention_196_only_block_and_reverse_walk(sig):
    e = sig[12]
    for n in (3, 60):  # hsplit 12 / 12 with 720 blocks: an uneven persistent walk
        qkv = _random_qkv(n, 12, 50 + n)
        try:
            for mode in MODES:
                e.set_attention_mode(mode)
                full, _ = e.attention(qkv, 0)
                rev, _ = e.attention(qkv, 0, reverse=True)
                assert _same(rev, full), (n, mode)
                for b in range(7) if n == 3 else (0, 6):
                    out = torch.full_like(full, -12345.0)
                    sentinel = out.clone()
                    e.attention(qkv, 0, only_block=b, out=out)
                    rows = torch.zeros(T, dtype=torch.bool, device=DEV)
                    rows[32 * b : 32 * b + 32] = True  # block 6: rows 192..195
                    rows = rows.repeat(n)
                    assert int(rows.sum()) == n * (32 if b < 6 else 4)
                    assert _same(out[rows], full[rows]), (n, mode, b)
                    assert _same(out[~rows], sentinel[~rows]), (n, mode, b)
        finally:
            e.set_attention_mode(1)
    with pytest.raises(MmeError):
        e.attention(qkv, 0, only_block=7)
    with pytest.raises(MmeError, match="contiguous bf16"):
        e.attention(_random_qkv(1, 12, 1, tokens=197), 0)  # 197 rows are no multiple of 196


def test_the_197_token_kernel_is_unaffected(sig):
    """A context that held a SigLIP tower and is reloaded with a CLIP tower runs the 197-token kernel again, and a fresh
    CLIP context gives the same bits; the same rows read as 196-token crops give another result."""
    from test_gpu_attention import _random_qkv as rq197
    from test_gpu_attention import check_close as check197
    from test_gpu_attention import reference as ref197

    g = dataclasses.replace(CLIP_B16, num_layers=1, intermediate_size=64, projection_dim=None)
    w = make_clip_weights(15, g)
    qkv = rq197(0, 3, 77, 0.25)
    ref, A = ref197(qkv, 0)
    e, fresh = Engine(0), Engine(0)
    try:
        e.load_siglip(make_siglip_weights(52, tiny(12)), tiny(12))
        a196, _ = e.attention(_random_qkv(3, 12, 77), 0)
        assert tuple(a196.shape) == (3 * 196, 768)
        e.load_clip(w, g)
        fresh.load_clip(w, g)
        for mode in MODES:
            e.set_attention_mode(mode)
            fresh.set_attention_mode(mode)
            out, _ = e.attention(qkv, 0)
            assert tuple(out.shape) == (3 * 197, 768)
            check197(out, ref, A, 0, f"197 tokens after a SigLIP load, mode {mode}")
            assert _same(out, fresh.attention(qkv, 0)[0])
    finally:
        e.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# (2) tanh-GELU epilogues


def tgelu_ref(x):
    """float64 tanh-GELU in the form that keeps its relative accuracy in the negative tail: x sigmoid(x (c0 + c1 x^2)), the
    identity tests/test_siglip_cpu.py holds to rounding.  (0.5 x (1 + tanh u) cancels there: 1 + tanh u keeps 2^-53 absolute,
    which is 1e-3 of a result of 1e-12 -- more than the bf16 rounding this file has to see.)"""
    return sr.gelu_tanh_sigmoid(x)


def tgelu_tol(ref, x):
    z = (x * (sr.C0 + sr.C1 * x * x)).abs() * (LOG2E / 2)
    return ulp_bf16(ref) / 2 * (1 + 2.0**-6) + 8 * 2.0**-24 * (1 + z) * ref.abs() + 2.0**-126


def tlaunch(eng, op, A, W, variant, bias, what):
    M, N = A.shape[0], W.shape[0]
    buf = Guard(BF16, M, N)
    kw = {}
    if op == 1:  # planted statistics (0, 1) and a zero colsum: the folded form reduces to acc + bias exactly
        st = torch.zeros((M, 2), dtype=F32, device=DEV)
        st[:, 1] = 1.0
        kw = dict(ln_stats=st, colsum=torch.zeros(N, dtype=F32, device=DEV))
    ran = eng.siglip_apply(op, A=A, W=W, variant=variant, bias=bias, out=buf.view, ldo=buf.ld, **kw)
    want = expect_256(variant, M, N, A.shape[1])
    assert ran == want, f"{what}: ran_256 = {ran}, expected {want}"
    buf.check(what)
    return buf.valid.clone()


@pytest.mark.parametrize("M", [257, 300])
@pytest.mark.parametrize("op", [0, 1])
def test_tanh_gelu_interior_tile_and_ragged_edge(eng, op, M):
    """N = 1536, K = 384: under variants 3 and 4 the 256 x 256 kernel has one row panel of interior tiles (the fast epilogue) and a
    ragged panel of 1 or 44 rows (epi_store); variant 1 is the 128 x 128 kernel.  Pre-activations N(0, ~2.5) + a bias."""
    N, K = 1536, 384
    g = _gen(90 + op + M)
    A, W = _randn((M, K), g, 1.0, BF16), _randn((N, K), g, 0.125, BF16)
    bias = _randn((N,), g, 0.5)
    acc = acc64(A, W)
    x = acc + bias.double()
    assert float(x.abs().max()) > 8 and float(x.min()) < -6
    grid = torch.linspace(-40, 40, 800001, dtype=F64, requires_grad=True)
    (slope,) = torch.autograd.grad(tgelu_ref(grid).sum(), grid)
    assert float(slope.abs().max()) < 1.13  # |d/dx gelu_tanh|
    core = torch.linspace(-4, 12, 100001, dtype=F64)
    assert float((tgelu_ref(core) - torch.nn.functional.gelu(core, approximate="tanh")).abs().max()) < 1e-14  # the same function
    ref = tgelu_ref(x)
    d = K * 2.0**-23 * absacc64(A, W) + 4 * 2.0**-24 * (acc.abs() + bias.double().abs())  # the f32 accumulation and the bias add
    tol = tgelu_tol(ref, x) + 1.13 * d
    outs = []
    for variant in (1, 3, 4):
        w = f"tanh-GELU op {op} M {M} variant {variant}"
        outs.append(tlaunch(eng, op, A, W, variant, bias, w))
        assert_close(outs[-1].double(), ref, tol, w)
    assert torch.equal(outs[0].view(I16), outs[1].view(I16)) and torch.equal(outs[1].view(I16), outs[2].view(I16))
    # (erf-GELU, at most 4.7e-4 away, is below this case's accumulation error; the exact grid below separates it)
    assert_mutant_far(x * torch.sigmoid(1.702 * x), ref, tol, 2000, "QuickGELU")
    assert_mutant_far(tgelu_ref(acc) + bias.double(), ref, tol, ref.numel() // 2, "bias added after the activation")


@pytest.mark.parametrize("op", [0, 1])
def test_tanh_gelu_dense_grid_and_the_tails(eng, op):
    """Every pre-activation exactly representable: acc = a_m * w_n with one non-zero product.  a: every bf16 value of
    [-12, -0.25], every third of [0.25, 12] and the tail values -100, -60, -12, 0, 12, +-inf (w = 1 in column 255)."""
    from test_gpu_gemm import _bf16_from_bits

    M, N, K = 1024, 256, 128
    special = torch.tensor([-100.0, -60.0, -12.0, 0.0, -0.0, 12.0, math.inf, -math.inf, 100.0, 3e38, -3e38, 2.0**-100], dtype=F64, device=DEV)
    a = torch.cat([-_bf16_from_bits(0x3E80, 0x4140), _bf16_from_bits(0x3E80, 0x4141, 3), -_bf16_from_bits(0x3D00, 0x3D00 + 4 * 73, 4), special]).to(BF16)
    assert a.numel() == M
    n = torch.arange(N, device=DEV, dtype=F64)
    w = torch.where(n < 128, 0.5 + n / 256, 0.25 + (n - 128) / 512)
    w[255] = 1.0
    A = torch.zeros((M, K), dtype=BF16, device=DEV)
    W = torch.zeros((N, K), dtype=BF16, device=DEV)
    A[:, 0], W[:, 0] = a, w.to(BF16)
    x = a.double()[:, None] * w[None, :]
    assert torch.equal(x.float().double()[torch.isfinite(x)], x[torch.isfinite(x)])
    core = x[x.abs() <= 12]
    assert int(torch.unique(core).numel()) >= 50_000
    bias = torch.zeros(N, dtype=F32, device=DEV)
    ref = tgelu_ref(x)
    ref[x == -math.inf] = 0.0  # the limit (torch's own float64 form returns NaN = -inf * 0 there)
    fin = torch.isfinite(x)
    tol = tgelu_tol(ref, torch.where(fin, x, torch.zeros_like(x)))
    outs = {}
    for variant in (1, 3, 4):  # 3, 4: four interior 256 x 256 tiles (fast path); 1: epi_store (slow path)
        what = f"tanh-GELU grid op {op} variant {variant}"
        out = outs[variant] = tlaunch(eng, op, A, W, variant, bias, what)
        o = out.double()
        assert_close(o[fin].reshape(1, -1), ref[fin].reshape(1, -1), tol[fin].reshape(1, -1), what)
        tail = {float(v): o[M - special.numel() + i, 255] for i, v in enumerate(special.tolist()) if not (v == 0 and i == 4)}
        sign = lambda t: bool(torch.signbit(t))  # noqa: E731
        for v in (-100.0, -60.0, -12.0, -math.inf, -3e38):  # the result is below every f32: -0, never NaN, never an inf
            assert float(tail[v]) == 0.0 and sign(tail[v]), (what, v, float(tail[v]))
        assert float(tail[0.0]) == 0.0 and float(tail[12.0]) == 12.0 and float(tail[100.0]) == 100.0
        assert float(tail[math.inf]) == math.inf and float(o[M - special.numel() + 9, 255]) == float(torch.tensor(3e38).to(BF16))
        assert float(o[M - special.numel() + 4, 255]) == 0.0  # -0 in
        col = o[:, 255]
        assert bool(torch.isfinite(col[a.double() != math.inf]).all()), what
    assert torch.equal(outs[1].view(I16), outs[3].view(I16)), "slow-path and fast-path tanh-GELU differ in bits"
    assert torch.equal(outs[4].view(I16), outs[3].view(I16))
    assert_mutant_far(gelu_ref(x)[fin], ref[fin], tol[fin], 2000, "erf-GELU")
    assert_mutant_far((x * torch.sigmoid(1.702 * x))[fin], ref[fin], tol[fin], 2000, "QuickGELU")


# ---------------------------------------------------------------------------------------------------------------------
# (3) embed_rows_t196


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [384, 768, 1024])
def test_embed_rows_t196_bit_for_bit(eng, d, n):
    g = _gen(70 + d + n)
    acc, bias, pos = _randn((n * T, d), g, 3.0), _randn((d,), g), _randn((T, d), g)
    x = Guard(BF16, n * T, d)
    eng.siglip_apply("embed_rows", acc=acc, bias=bias, pos=pos, x=x.view, n=n, d=d)
    x.check("embed_rows_t196")
    a, b, p = (t.cpu().numpy() for t in (acc, bias, pos))
    want32 = (a.reshape(n, T, d) + b[None, None]) + p[None]  # numpy float32: (acc + bias) + pos, IEEE additions
    want = torch.from_numpy(want32.reshape(n * T, d)).to(DEV).to(BF16).view(I16)  # round to nearest even
    assert_bits(x.valid_bits(), want, f"embed_rows_t196 d {d} n {n}")
    mut = a.reshape(n, T, d) + (b[None, None] + p[None])
    assert int((torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16) != want).sum()) > 0, "the order of the additions does not show"
    mut = (a.reshape(n, T, d) + b[None, None]) + np.roll(p, 1, axis=0)[None]
    assert_mutant_bits(torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16), want, n * T * d // 2, "pos[p - 1] for pos[p]")
    if n > 1:  # the 197-token pitch: the position row shifts by one per crop
        rows = np.arange(n * T)
        mut = (a + b[None]) + p[(rows - rows // 197) % T]
        assert_mutant_bits(torch.from_numpy(mut).to(DEV).to(BF16).view(I16)[T:], want[T:], (n - 1) * T * d // 4, "a crop every 197 rows")


# ---------------------------------------------------------------------------------------------------------------------
# (4) map_pool


def pool_reference(kv, q, H, mutant=None):
    """float64 (out, A), each [n, H * dh]: per (crop, head) softmax_j(q_h . k_j) in base 2 over the 196 keys, times V"""
    x = kv.view(-1, T, 2, H, DH).double()
    k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)  # [n, H, T, dh]
    s = (k * q.double().view(1, H, 1, DH)).sum(-1)  # [n, H, T]
    if mutant:
        s = mutant(s)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    out = (p[..., None] * v).sum(2) / l
    A = (p[..., None] * v.abs()).sum(2) / l
    n = x.shape[0]
    return out.reshape(n, H * DH), A.reshape(n, H * DH)


def run_pool(eng, kv, q, H, what):
    n = kv.shape[0] // T
    out = Guard(BF16, n, H * DH)
    eng.siglip_apply("map_pool", kv=kv, q=q, out=out.view, n=n, heads=H)
    out.check(what)
    return out.valid.clone()


def _random_kv(n, H, seed, extra_rows=1):
    """K | V ~ N(0, 1) in bf16 behind n * 196 rows, then `extra_rows` rows of NaN: what a read past the last row would meet"""
    g = _gen(seed)
    big = torch.full((n * T + extra_rows, 2 * H * DH), float("nan"), dtype=BF16, device=DEV)
    big[: n * T] = _randn((n * T, 2 * H * DH), g, 1.0, BF16)
    return big[: n * T]


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("H", [6, 12, 16])
def test_map_pool_random(eng, H, n):
    kv = _random_kv(n, H, 600 + H + n)
    q = _randn((H * DH,), _gen(7 + H), 0.35)  # scores with a standard deviation of ~2.8 log2 units
    ref, A = pool_reference(kv, q, H)
    got = run_pool(eng, kv, q, H, f"map_pool random H {H} n {n}")
    tol = _tol(ref, A)
    assert_close(got.double(), ref, tol, f"map_pool random H {H} n {n}")
    x = kv.view(n, T, 2, H, DH).double()
    assert_mutant_far(x[:, :, 1].mean(1).reshape(n, H * DH), ref, tol, n * H * DH // 2, "the plain mean (scores ignored)")
    sw, _ = pool_reference(kv, q.view(H, DH).roll(1, 0).reshape(-1), H)
    assert_mutant_far(sw, ref, tol, n * H * DH // 2, "the query of the neighbouring head")
    nat, _ = pool_reference(kv, q * (1 / LOG2E), H)
    assert_mutant_far(nat, ref, tol, n * H * DH // 4, "exp for exp2")


@pytest.mark.parametrize("H", [6, 12, 16])
def test_map_pool_zero_query_is_the_mean_and_spikes_return_their_row(eng, H):
    n = 3
    kv = _random_kv(n, H, 700 + H)
    x = kv.view(n, T, 2, H, DH)
    q = torch.zeros(H * DH, dtype=F32, device=DEV)
    ref, A = pool_reference(kv, q, H)
    mean = x[:, :, 1].double().mean(1).reshape(n, H * DH)
    assert bool(((ref - mean).abs() <= 1e-12 * A).all())
    got = run_pool(eng, kv, q, H, f"map_pool q = 0, H {H}")
    assert_close(got.double(), ref, _tol(ref, A), f"map_pool q = 0, H {H}")
    v = x[:, :, 1].double()
    counted = ((v.sum(1) + 60 * v[:, 195]) / 256).reshape(n, H * DH)  # lanes 4..63 of the fourth round as copies of key 195
    assert_mutant_far(counted, ref, _tol(ref, A), n * H * DH // 2, "keys 196..255 counted")
    # spikes: q = e_0 of every head, dim 0 of K zero except 40 at the spike key: the other keys weigh 2^-40 each
    keys = (0, 63, 64, 195)
    q = torch.zeros(H * DH, dtype=F32, device=DEV)
    q.view(H, DH)[:, 0] = 1.0
    x[:, :, 0, :, 0] = 0.0
    key_of = torch.tensor([[keys[(i * H + h) % 4] for h in range(H)] for i in range(n)], device=DEV)
    for i in range(n):
        for h in range(H):
            x[i, int(key_of[i, h]), 0, h, 0] = 40.0
    want = torch.stack([torch.stack([x[i, int(key_of[i, h]), 1, h] for h in range(H)]) for i in range(n)]).reshape(n, H * DH)
    got = run_pool(eng, kv, q, H, f"map_pool spikes, H {H}")
    assert_bits(got.view(I16), want.view(I16), f"map_pool spikes H {H}: the spike key's value row")
    ref, A = pool_reference(kv, q, H)
    onehot = torch.nn.functional.one_hot(key_of, T).bool()
    mref, _ = pool_reference(kv, q, H, lambda s: s.masked_fill(onehot, float("-inf")))
    assert_mutant_far(mref, ref, _tol(ref, A), n * H * DH // 2, "the spike key dropped")


@pytest.mark.parametrize("H", [6, 12, 16])
def test_map_pool_huge_scores_stay_finite(eng, H):
    """|k| = 1e30 at keys 7 and 195 in dim 0, q_0 = 3e7: scores of +-3e37, finite in f32; the exact maximum keeps every
    exponential at or below 1."""
    n = 2
    kv = _random_kv(n, H, 800 + H)
    x = kv.view(n, T, 2, H, DH)
    x[:, 7, 0, :, 0] = 1e30
    x[:, 195, 0, :, 0] = -1e30
    x[:, :, 0, :, 1:] = 0.0
    q = torch.zeros(H * DH, dtype=F32, device=DEV)
    q.view(H, DH)[:, 0] = 3e7
    q.view(H, DH)[1::2, 0] = -3e7  # odd heads: key 195 wins
    ref, A = pool_reference(kv, q, H)
    assert bool(torch.isfinite(ref).all())
    got = run_pool(eng, kv, q, H, f"map_pool huge scores, H {H}")
    assert_close(got.double(), ref, _tol(ref, A), f"map_pool huge scores, H {H}")
    want = torch.stack([x[:, 7 if h % 2 == 0 else 195, 1, h] for h in range(H)], 1).reshape(n, H * DH)
    assert_bits(got.view(I16), want.view(I16), "map_pool huge scores: the winning key's value row")


# ---------------------------------------------------------------------------------------------------------------------
# (5) l2_rows_bf16


@pytest.mark.parametrize("d", [384, 768, 1024])
@pytest.mark.parametrize("n", [1, 5])
def test_l2_rows_bf16(eng, n, d):
    rng = np.random.default_rng(900 + d + n)
    xh = rng.standard_normal((n, d)).astype(np.float32)
    if n > 1:
        xh[1] *= 1e4
        xh[2] *= 1e-4
        xh[3] = 0.0  # zero row: stays zero (the 1e-12 floor)
    X = torch.from_numpy(xh).to(DEV).to(BF16)
    o32, o16 = Guard(F32, n, d), Guard(BF16, n, d)
    eng.siglip_apply("l2_bf16", x=X, emb_f32=o32.view, emb_bf16=o16.view, n=n, d=d)
    o32.check("l2_rows_bf16 f32")
    o16.check("l2_rows_bf16 bf16")
    got = o32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(o16.valid_bits(), got.to(BF16).view(I16), "l2_rows_bf16: bf16 output vs RNE of the f32 output")
    rows = X.float().cpu().numpy()
    ref = l2_ref_np(rows, np.float64)
    yard = float(np.abs(l2_ref_np(rows, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print(f"l2_rows_bf16 n {n} d {d}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    if n > 1:
        assert float(got[3].abs().max()) == 0.0
        assert int((np.abs(l2_ref_np(np.roll(rows, 1, axis=0), np.float64) - ref) > 4 * tol).sum()) >= n * d // 2, "mutant 'the row before' not separated"
    only = Guard(BF16, n, d)
    eng.siglip_apply("l2_bf16", x=X, emb_bf16=only.view, n=n, d=d)
    assert torch.equal(only.valid_bits(), o16.valid_bits())


# ---------------------------------------------------------------------------------------------------------------------
# (6) prepared buffers


def _as_vit_names(m, g):
    """the tower's tensors under the ViT names of tests/test_gpu_weight_prep.py's table (layer_norm1 -> layernorm_before, ...)"""
    v = "vision_model."
    o = {"embeddings.cls_token": None, "embeddings.position_embeddings": m[v + "embeddings.position_embedding.weight"],
         "embeddings.patch_embeddings.projection.weight": m[v + "embeddings.patch_embedding.weight"],
         "embeddings.patch_embeddings.projection.bias": m[v + "embeddings.patch_embedding.bias"], "layernorm.weight": m[v + "post_layernorm.weight"],
         "layernorm.bias": m[v + "post_layernorm.bias"]}
    for l in range(g.num_layers):
        p, q = f"{v}encoder.layers.{l}.", f"layers.{l}."
        for wb in ("weight", "bias"):
            o[q + "layernorm_before." + wb] = m[p + "layer_norm1." + wb]
            o[q + "layernorm_after." + wb] = m[p + "layer_norm2." + wb]
            for a, b in (("q_proj", "q_proj"), ("k_proj", "k_proj"), ("v_proj", "v_proj"), ("o_proj", "out_proj")):
                o[q + f"attention.{a}.{wb}"] = m[p + f"self_attn.{b}.{wb}"]
            o[q + "mlp.fc1." + wb] = m[p + "mlp.fc1." + wb]
            o[q + "mlp.fc2." + wb] = m[p + "mlp.fc2." + wb]
    return o


@pytest.mark.parametrize("case", [("bfloat16", SiglipGeometry(hidden_size=384, num_layers=2, num_heads=6, intermediate_size=128)),
                                  ("float16", SiglipGeometry(hidden_size=1024, num_layers=1, num_heads=16, intermediate_size=64)),
                                  ("float32", SiglipGeometry(hidden_size=768, num_layers=1, num_heads=12, intermediate_size=64))],
                         ids=["384x2-bf16", "1024x1-f16", "768x1-f32"])
def test_prepared_buffers(tmp_path, case):
    """Both preparers against float64 from the weights: the split of in_proj (q | k | v by rows), K | V unfolded and with
    post_layernorm folded in (W', column sums, bias'), the constant query, the head's MLP."""
    import test_gpu_weight_prep as wp

    dtype, geom = case
    ckpt.save_checkpoint(tmp_path, make_siglip_weights(21, geom), "siglip", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "siglip")
    assert ck.dtype == dtype and ck.geometry == geom
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_siglip_checkpoint(ck)
        host.load_siglip({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (bd, fd), (bh, fh) = wp._read_all(dev), wp._read_all(host)
        info = dev.encoder_info()
    finally:
        dev.close()
        host.close()
    assert info == {"kind": "siglip", "embed_dim": geom.hidden_size, "hidden_act": "gelu_pytorch_tanh", "projection_dim": None}
    D, L = geom.hidden_size, geom.num_layers
    assert len(bd) == len(bh) == 6 + 18 * L + 19 and fd == fh
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    assert bd[1].size == 4 * T * D  # pos f32 [196, D]
    wp.DEV_OF[0] = DEV
    m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    table = wp.vit_table(_as_vit_names(m, geom), geom)
    assert table[0][0] == "cls"
    table[0] = ("cls", "zeros", D)
    h = "vision_model.head."
    wi, bi = m[h + "attention.in_proj_weight"], m[h + "attention.in_proj_bias"]
    lnf_g, lnf_b = m["vision_model.post_layernorm.weight"], m["vision_model.post_layernorm.bias"]
    sc = geom.head_dim**-0.5 * LOG2E

    def head_table(split=(0, 1, 2), probe=None):
        q, k, v = (wi[i * D : (i + 1) * D] for i in split)
        qb, kb, vb = (bi[i * D : (i + 1) * D] for i in split)
        kvd = dict(W=[k, v], b=[kb, vb], s=[None, None], gamma=lnf_g, beta=lnf_b, eps=geom.layer_norm_eps)
        qd = dict(W=[q], b=[qb], s=[sc], gamma=lnf_g, beta=m[h + "probe"].reshape(D) if probe is None else probe, eps=geom.layer_norm_eps)
        fc1 = dict(W=[m[h + "mlp.fc1.weight"]], b=[m[h + "mlp.fc1.bias"]], s=[None], gamma=m[h + "layernorm.weight"], beta=m[h + "layernorm.bias"],
                   eps=geom.layer_norm_eps)
        return [("h.ln2_g", "f32", m[h + "layernorm.weight"]), ("h.ln2_b", "f32", m[h + "layernorm.bias"]),
                ("h.kv_w", "bf16", torch.cat([k, v])), ("h.kv_b", "f32", torch.cat([kb, vb])),
                ("h.kv_wf", "fold", kvd), ("h.kv_cs", "cs", kvd), ("h.kv_bf", "bf", kvd),
                ("h.q_wf", "fold", qd), ("h.q_cs", "cs", qd), ("h.q", "bf", qd),
                ("h.o_w", "bf16", m[h + "attention.out_proj.weight"]), ("h.o_b", "f32", m[h + "attention.out_proj.bias"]),
                ("h.fc1_w", "bf16", m[h + "mlp.fc1.weight"]), ("h.fc1_b", "f32", m[h + "mlp.fc1.bias"]),
                ("h.fc1_wf", "fold", fc1), ("h.fc1_cs", "cs", fc1), ("h.fc1_bf", "bf", fc1),
                ("h.fc2_w", "bf16", m[h + "mlp.fc2.weight"]), ("h.fc2_b", "f32", m[h + "mlp.fc2.bias"])]

    head = head_table()
    assert len(head) == 19
    folds = wp.check_table(table + head, bd, f"siglip {dtype}")
    assert len(folds) == 2 * L + 3
    # the constant query once more, from its definition alone: (probe . W_q^T + b_q) dh^-0.5 log2 e
    iq = len(table) + 9
    got_q = torch.from_numpy(bd[iq].view(np.float32).copy()).to(DEV).double()
    ref_q = (m[h + "probe"].reshape(1, D).double() @ wi[:D].double().T + bi[:D].double()).reshape(D) * sc
    mag = (m[h + "probe"].reshape(1, D).double().abs() @ wi[:D].double().abs().T + bi[:D].double().abs()).reshape(D) * sc
    tol_q = wp.ulp_f32(ref_q) / 2 + 2.0**-22 * mag  # the scale is applied in f32 to every weight first
    assert_close(got_q[None], ref_q[None], tol_q[None], "the constant query")
    assert_mutant_far((ref_q / LOG2E)[None], ref_q[None], tol_q[None], D // 2, "scale without log2(e)")
    assert_mutant_far((ref_q + m[h + "probe"].reshape(D).double())[None], ref_q[None], tol_q[None], D // 2, "the probe added")
    # mutants of the split: q | v | k, and k | q | v -- each leaves the read-back buffers on most elements
    kv_bits = torch.from_numpy(bd[len(table) + 2].view(np.int16).copy()).to(DEV)
    for split, name in (((0, 2, 1), "K and V exchanged"), ((1, 0, 2), "Q and K exchanged")):
        mt = head_table(split)
        want = wp.bf16_rne(mt[2][2].float().reshape(-1))
        assert int((want != kv_bits).sum()) >= kv_bits.numel() // 4, f"mutant '{name}' is not separated on K | V"


# ---------------------------------------------------------------------------------------------------------------------
# (7) end to end


@pytest.mark.parametrize("key", ["B16s", "S16", "L16"])
def test_end_to_end_against_the_restatement_and_transformers(golden_dir, key):
    from oracle import preprocess as opre

    seed, geom = CASES[key]
    w = weights_of(key)
    arrays = list(synthetic_crops(mks.N_CROPS, seed=0)) + _golden_crops(golden_dir)
    assert len(arrays) == 40
    pv = np.stack([opre.preprocess_crop(a) for a in arrays]).astype(np.float32)
    emb = RegionEmbedder(device=0, encoder="siglip_vit", weights=w, geometry=geom, chunk=64)
    try:
        assert emb.embed_dim == geom.hidden_size and emb.engine.encoder_info()["kind"] == "siglip"
        pix, offs, hw = _pack(arrays)
        e32, e16 = emb.embed_packed(pix, offs, hw)
        torch.cuda.synchronize()
        assert emb.engine.attention_redone(geom.num_layers) == [0] * geom.num_layers
        got = e32.cpu().numpy()
        assert got.shape == (40, geom.hidden_size) and np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)
        assert rows.shape == (3, geom.hidden_size) and ok.all() and np.array_equal(rows, got[:3])
        with pytest.raises(NotImplementedError):
            emb.get_text_embeddings("a query")
    finally:
        _close_all(emb)
    want = sr.siglip_embed(pv, w, geom, torch.float32)
    omc = sr.one_minus_cos(got, want)
    print(f"siglip parity {key} ({geom.hidden_size}-d x {geom.num_layers} layers): max(1 - cos) = {omc.max():.3g} "
          f"(synthetic 224^2: {omc[:16].max():.3g}, bundled: {omc[16:].max():.3g})")
    assert float(omc.max()) <= 1e-3, (key, float(omc.max()))
    mu = want.mean(axis=0, keepdims=True)
    a, b = got - mu, want - mu  # centred: near-identical seeded-weight embeddings cannot pass trivially
    ccos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    print(f"siglip parity {key}: centred cosine min = {ccos.min():.4f}")
    assert np.all(ccos > 0.98), (key, float(ccos.min()))
    rec = np.load(os.path.join(golden_dir, "siglip_cases.npz"))[f"{key}.pooler_output"]
    omc_hf = sr.one_minus_cos(got[:16], rec)
    print(f"siglip parity {key}: against the recorded transformers rows max(1 - cos) = {omc_hf.max():.3g}")
    assert float(omc_hf.max()) <= 1e-3, (key, float(omc_hf.max()))


def test_region_embedder_seeded_default_reports_768_and_unit_vectors(caplog):
    import logging

    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        emb = RegionEmbedder("no-such/siglip-checkpoint", device=0, chunk=64, encoder="siglip_vit", geometry=dataclasses.replace(SIGLIP_B16, num_layers=2))
    try:
        assert any("SEEDED SYNTHETIC" in r.getMessage() for r in caplog.records)
        assert emb.embed_dim == 768 and emb.pool_token == 0
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(3, seed=8)), as_array=True)
        assert ok.all() and rows.shape == (3, 768) and np.allclose(np.linalg.norm(rows, axis=1), 1.0, atol=1e-5)
    finally:
        _close_all(emb)
    emb = RegionEmbedder(device=0, chunk=64, encoder="siglip_vit")
    try:
        g = emb.engine.vit_geometry()
        assert emb.embed_dim == 768 and (g.hidden_size, g.num_layers, g.num_heads, g.intermediate_size, g.patch_size) == (768, 12, 12, 3072, 16)
    finally:
        _close_all(emb)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_checkpoint_directory_equals_weights_dict(tmp_path, crops40, dtype):
    geom, w = CASES["S16"][1], weights_of("S16")
    ckpt.save_checkpoint(tmp_path, w, "siglip", dtype, geometry=geom, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5),
                         image_processor_type="SiglipImageProcessor")
    by_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="siglip_vit")
    ck = by_dir.checkpoint
    by_dict = RegionEmbedder(device=0, chunk=64, encoder="siglip_vit", weights={k: t.float().numpy() for k, t in ck.tensors.items()}, geometry=geom)
    try:
        by_dict.engine.set_normalisation((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        assert ck.geometry == geom and ck.dtype == dtype and by_dir.embed_dim == by_dict.embed_dim == 384
        assert by_dir.engine.weights_fingerprint() == by_dict.engine.weights_fingerprint()
        a32, a16 = by_dir.embed_uniform(crops40)
        b32, b16 = by_dict.embed_uniform(crops40)
        torch.cuda.synchronize()
        assert torch.equal(a32, b32) and torch.equal(a16, b16) and bool(torch.isfinite(a32).all()) and tuple(a32.shape) == (40, 384)
    finally:
        _close_all(by_dir)
        _close_all(by_dict)


@pytest.mark.parametrize("key", ["S16", "B16s", "L16"])
def test_forward_settings_are_bit_identical(crops40, key):
    """As the tests of this name at 197 and 50 tokens: the two folded LayerNorm modes (1: one statistics pass over x, 2: partial
    sums from the producing GEMM), every GEMM variant, chunking, the tile order, pruning (without effect) and the three
    attention modes give the same bits.  300 crops = 58 800 rows: interior 256-row tiles and a ragged one."""
    geom = CASES[key][1]
    eng = Engine(0)
    try:
        eng.load_siglip(weights_of(key), geom)
        crops = torch.cat([crops40, torch.from_numpy(synthetic_crops(260, seed=9)).cuda()])
        eng.set_chunk(300)
        eng.set_ln_fusion(1)
        ref, _ = _uniform(eng, crops)
        assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (300, geom.hidden_size)
        for variant in (0, 1, 3, 4, 6):
            eng.set_gemm_variant(variant)
            for mode in (2, 1):
                eng.set_ln_fusion(mode)
                got, _ = _uniform(eng, crops)
                assert torch.equal(ref, got), (key, "gemm variant", variant, "ln fusion", mode)
        eng.set_gemm_variant(0)
        eng.set_ln_fusion(2)
        eng.set_forward_pruning(True)
        for tok in (0, 195):  # the token is ignored and pruning has no effect
            got, _ = _uniform(eng, crops, tok)
            assert torch.equal(ref, got), (key, "pruning, pool_token", tok)
        eng.set_forward_pruning(False)
        eng.set_chunk(64)
        c64, _ = _uniform(eng, crops40)
        eng.set_chunk(8)
        c8, _ = _uniform(eng, crops40)
        assert torch.equal(c64, c8), (key, "chunk 64 vs 8")
        assert torch.equal(c64, ref[:40]), (key, "the same crops inside a pass of 300")
        for order in (0, 2, 1):
            eng.set_tile_order(order)
            got, _ = _uniform(eng, crops40)
            assert torch.equal(got, c8), (key, "tile order", order)
        # the forced exact re-run of every attention launch against the exact form; the fast form within its own rounding
        eng.set_attention_mode(0)
        exact, _ = _uniform(eng, crops40)
        assert eng.attention_redone(geom.num_layers) == [0] * geom.num_layers
        eng.set_attention_mode(2)
        forced, _ = _uniform(eng, crops40)
        assert eng.attention_redone(geom.num_layers) == [1] * geom.num_layers
        eng.set_attention_mode(1)
        assert torch.equal(exact, forced), (key, "attention mode 2 vs 0")
        fast, _ = _uniform(eng, crops40)
        assert eng.attention_redone(geom.num_layers) == [0] * geom.num_layers and torch.equal(fast, c8)
        assert float((1.0 - (fast * exact).sum(dim=1)).max()) <= 1e-4
        with pytest.raises(MmeError, match="pool_token 196 outside 0..195"):
            _uniform(eng, crops40, 196)
    finally:
        eng.close()


def test_layernorm_kernel_mode_against_the_restatement():
    """ln_fusion 0: LayerNorm kernels, the unfolded K | V GEMM and the unfolded fc1 epilogue (EPI_BIAS_TGELU); the same bound.
    (Mode 0 rounds the normalised rows to bf16 where the folded modes do not: as at 197 and 50 tokens it is held to the
    bf16 budget, and to the folded modes within that budget, not to their bits.)"""
    from oracle import preprocess as opre

    geom, w = CASES["S16"][1], weights_of("S16")
    crops = synthetic_crops(16, seed=0)
    pv = np.stack([opre.preprocess_crop(a) for a in crops]).astype(np.float32)
    eng = Engine(0)
    try:
        eng.load_siglip(w, geom)
        eng.set_chunk(64)
        eng.set_ln_fusion(0)
        got0 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
        eng.set_ln_fusion(2)
        got2 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
    finally:
        eng.close()
    want = sr.siglip_embed(pv, w, geom, torch.float32)
    omc0, omc02 = sr.one_minus_cos(got0, want), sr.one_minus_cos(got0, got2)
    print(f"siglip parity S16, LayerNorm-kernel mode: max(1 - cos) = {omc0.max():.3g}; against the folded mode {omc02.max():.3g}")
    assert float(omc0.max()) <= 1e-3 and float(omc02.max()) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# (8) coexistence and refusals


def test_clip_then_siglip_then_clip_on_one_context(crops40):
    g16 = dataclasses.replace(CLIP_B16, num_layers=2)
    gs = CASES["B16s"][1]
    w16, ws = make_clip_weights(15, g16), weights_of("B16s")
    fresh = Engine(0)
    try:
        fresh.load_siglip(ws, gs)
        fresh.set_chunk(64)
        solo = [t.clone() for t in _uniform(fresh, crops40)]
    finally:
        fresh.close()
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.set_forward_pruning(True)
        e.load_clip(w16, g16)
        first = [t.clone() for t in _uniform(e, crops40)]
        fp16 = e.weights_fingerprint()
        p16 = e.preprocess(*_pack(list(synthetic_crops(2, seed=1))))
        e.load_siglip(ws, gs)
        assert e.encoder_info() == {"kind": "siglip", "embed_dim": 768, "hidden_act": "gelu_pytorch_tanh", "projection_dim": None}
        second = _uniform(e, crops40)
        assert torch.equal(second[0], solo[0]) and torch.equal(second[1], solo[1])
        ps = e.preprocess(*_pack(list(synthetic_crops(2, seed=1))))
        assert tuple(ps.shape) == (2 * 196, 768) and torch.equal(ps.view(I16), p16.view(I16))  # K1 is the patch-16 K1
        sep = e.vit_forward(e.preprocess(*_pack(list(synthetic_crops(40, seed=3)))))  # preprocess -> forward equals embed
        torch.cuda.synchronize()
        assert torch.equal(sep[0], solo[0])
        e.load_clip(w16, g16)
        assert e.encoder_info()["kind"] == "clip" and e.weights_fingerprint() == fp16
        third = _uniform(e, crops40)
        assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
        assert not torch.equal(first[0][:, :512], second[0][:, :512])
    finally:
        e.close()


def test_text_tower_range_is_untouched_by_a_siglip_load(crops40):
    from test_gpu_clip_text import T2

    from multimodal_embeddings_amd.weights import make_clip_text_weights, synthetic_token_ids

    ids = synthetic_token_ids(4, T2.vocab_size, T2.eos_token_id, 13, [2, 20, 64, 77])
    tw = make_clip_text_weights(41, T2)
    gs = CASES["S16"][1]
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip_text(tw, T2)
        t0 = e.text_forward(ids, want_bf16=False)[0].clone()
        n_txt = len(e.weights_fingerprint())
        e.load_siglip(weights_of("S16"), gs)
        assert len(e.weights_fingerprint()) == n_txt + 6 + 18 * gs.num_layers + 19
        img0 = _uniform(e, crops40)[0].clone()
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32))
        g16 = dataclasses.replace(CLIP_B16, num_layers=1)
        e.load_clip(make_clip_weights(15, g16), g16)
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32))
        e.load_siglip(weights_of("S16"), gs)
        assert torch.equal(_uniform(e, crops40)[0], img0) and torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32))
    finally:
        e.close()


def test_refusals_leave_the_previous_weights_in_place(crops40):
    geom, w = CASES["S16"][1], weights_of("S16")
    eng = Engine(0)
    try:
        eng.load_siglip(w, geom)
        eng.set_chunk(64)
        before = [t.clone() for t in _uniform(eng, crops40)]
        fp = eng.weights_fingerprint()
        keep = {}

        def arr(name, first=0):
            if name not in keep:
                keep[name] = np.ascontiguousarray(w[name], dtype=np.float32).reshape(-1)
            return keep[name][first:].ctypes.data_as(C.POINTER(C.c_float))

        def refused(change, text):
            W, layers = eng._weights_struct("siglip", geom, arr)
            change(W)
            rc = eng.lib.mme_load_siglip(eng.h, C.byref(W))
            msg = eng.lib.mme_last_error(eng.h).decode()
            assert rc == -1 and text in msg, (rc, msg)
            assert eng.weights_fingerprint() == fp and eng.encoder_info()["kind"] == "siglip"

        for patch in (14, 32):
            refused(lambda W, p=patch: setattr(W.vit, "patch_size", p), f"mme_load_siglip: patch_size = {patch}; supported: 16")
        refused(lambda W: setattr(W.vit, "image_size", 256), "image_size = 256; supported: 224")
        refused(lambda W: setattr(W.vit, "hidden", 512), "hidden = 512; supported: 384, 768, 1024")
        refused(lambda W: setattr(W.vit, "heads", 8), "heads = 8 at hidden = 384; supported: heads of 64")
        refused(lambda W: setattr(W.vit, "mlp", 100), "mlp = 100; supported: multiples of 64 up to 8192")
        refused(lambda W: setattr(W.vit, "layers", 65), "layers = 65; supported: 1..64")
        refused(lambda W: setattr(W.vit, "cls_token", arr("vision_model.head.probe")), "vit.cls_token is set; supported: NULL")
        refused(lambda W: setattr(W, "probe", None), "probe is a null tensor pointer")
        refused(lambda W: setattr(W.head, "fc2_b", None), "head has a null tensor pointer")
        for act, field in (("gelu", "hidden_act"), ("quick_gelu", "hidden_act")):
            with pytest.raises(MmeError, match=f"{field} = '{act}'; supported: gelu_pytorch_tanh"):
                eng.load_siglip(w, dataclasses.replace(geom, hidden_act=act))
        with pytest.raises(MmeError, match="vision_use_head = False; supported: True"):
            eng.load_siglip(w, dataclasses.replace(geom, vision_use_head=False))
        with pytest.raises(MmeError, match="load_siglip: tensor 'vision_model.head.probe' is missing"):
            eng.load_siglip({k: v for k, v in w.items() if not k.endswith("head.probe")}, geom)
        assert eng.weights_fingerprint() == fp
        e32, e16 = _uniform(eng, crops40)
        assert torch.equal(e32, before[0]) and torch.equal(e16, before[1])
    finally:
        eng.close()


def test_siglip_apply_refuses_bad_arguments(eng):
    d, n, H = 768, 2, 12
    g = _gen(2)
    bias, q = _randn((d,), g), _randn((d,), g)
    acc, pos = _randn((n * T + 1, d), g), _randn((T, d), g)
    x, out, y = Guard(BF16, n * T, d), Guard(BF16, n, d), Guard(F32, n, d)
    kv = _random_kv(n, H, 3)
    A, W = _randn((64, 128), g, 1.0, BF16), _randn((64, 128), g, 1.0, BF16)
    gout = Guard(BF16, 64, 64)
    cases = [
        (dict(op=5, kv=kv, q=q, out=out.view, n=n, heads=H), "op 5 outside 0..4"),
        (dict(op=-1, kv=kv, q=q, out=out.view, n=n, heads=H), "op -1 outside 0..4"),
        (dict(op=0), "op 0 needs gemm"),
        (dict(op=0, A=A, W=W, bias=bias, out=gout.view, ldo=60), "ldo = 60 must be a multiple of 8"),
        (dict(op=1, A=A, W=W, bias=bias, out=gout.view), "op 1 needs ln_stats and colsum"),
        (dict(op=0, A=A[:, :32], W=W[:, :32], K=32, bias=bias, out=gout.view), "K = 32 must be a multiple of 64"),
        (dict(op=2, acc=acc, bias=bias, pos=pos, x=x.view, n=-1, d=d), "n = -1 outside"),
        (dict(op=2, acc=acc, bias=bias, pos=pos, x=x.view, n=n, d=512), "built for d == 384, d == 768 and d == 1024 (d = 512)"),
        (dict(op=2, acc=acc, bias=bias, x=x.view, n=n, d=d), "acc, bias, pos, x non-null and 16-byte aligned"),
        (dict(op=2, acc=acc.reshape(-1)[1:], bias=bias, pos=pos, x=x.view, n=n, d=d), "16-byte aligned"),
        (dict(op=3, kv=kv, q=q, out=out.view, n=n, heads=8), "built for heads == 6, 12 and 16 (heads = 8)"),
        (dict(op=3, kv=kv, out=out.view, n=n, heads=H), "kv, q and out non-null and 16-byte aligned"),
        (dict(op=3, kv=kv, q=q.reshape(-1)[1:], out=out.view, n=n, heads=H), "kv, q and out non-null and 16-byte aligned"),
        (dict(op=4, x=x.view, n=n, d=d), "emb_f32 or emb_bf16"),
        (dict(op=4, x=x.view, emb_f32=y.view.reshape(-1)[1:], n=n, d=d), "emb_f32 and emb_bf16 16-byte aligned"),
        (dict(op=4, emb_f32=y.view, n=n, d=d), "x non-null and 16-byte aligned"),
        (dict(op=4, x=x.view, emb_f32=y.view, n=n, d=1280), "(d = 1280)"),
    ]
    for kw, text in cases:
        op = kw.pop("op")
        with pytest.raises(MmeError) as ei:
            eng.siglip_apply(op, **kw)
        assert "(-1)" in str(ei.value) and text in str(ei.value), (op, text, str(ei.value))
    for buf in (x, out, y, gout):
        assert buf.untouched()
    # the 196-token attention needs a SigLIP context: a bare context runs 197 tokens
    with pytest.raises(MmeError, match="contiguous bf16"):
        eng.attention(_random_qkv(1, 12, 1), 0)
