"""The SigLIP text tower on the GPU (csrc/text_tower.hip, attention_short.hip, capi_text.hip): every new kernel one launch at a
time against numpy / float64, the prepared buffers of the two loaders, parity with what transformers returned
(tests/golden/siglip_text_cases.npz), coexistence with the CLIP text tower and the image towers, the public interface and the
refusals.

Tolerances, none fitted:
(1) token rows at 64 positions: bit-equal to bf16(f32 + f32) -- one add, one rounding to nearest even.
(2) attention, 64 tokens, no mask: |got - ref| <= 2^-8 |ref| + 2^-8 A, A = sum p |v| / sum p from the same float64 pass: the
    bound tests/test_gpu_attention.py derives for a kernel that rounds P to bf16 before P . V and the output to bf16, which are
    this kernel's two rounding points as well.  Items (n x heads): 8 (one sequence -- a launch of 1 item cannot be had, the
    kernel is built for 8, 12 and 16 heads), 12, and 1032 / 1040 (more than the 1024 persistent workgroups: some walk a second
    item; 25 MB of Q | K | V at 12 heads).
(3) last-row pool-LN: bit-equal to the 77-token kernel on the same rows (one template, the same f32 order), and the yardstick
    rule of tests/test_gpu_clip_text.py against float64: 8 x the deviation of a float32 numpy restatement, never below 2^-22 of
    the largest value, plus the bf16 format's own ulp / 2.
(4) bias_l2_rows: bit-equal to l2_rows on acc + bias formed in f32 (y is formed once in f32; the reduction order is l2_rows'),
    and tests/test_gpu_clip.py's l2_rows bound against float64.
(5) siglip_scores, p = 1 / (1 + exp(-(c s + b))), s = exp(logit_scale) formed on the host in f32.  Operation count in f32:
      s      one host expf: relative error <= 2^-23 (1 ulp);
      c s    one multiply: relative 2^-24;
      z      one add: relative 2^-24 of z.        So |dz| <= |c s| (2^-23 + 2^-24) + 2^-24 |z| <= 2^-22 |c s| + 2^-24 |z|.
      e      one exp of -z: relative error <= |dz| + 2^-22 (the library's expf within 2 ulp);
      1 + e  one add: relative 2^-24;   1 / (1 + e)  one reciprocal: relative <= 2^-23.
    dp / de = -p^2, so the error of e moves p by p (1 - p) rel(e); the last two steps move it by p (2^-24 + 2^-23):
      |got - ref| <= p (1 - p) (2^-22 |c s| + 2^-24 |z| + 2^-22) + 2^-22 p + 2^-126,
    the last term for results below the smallest normal f32, which the exp's overflow (z < -88.7: e = inf, p = 0) or a
    flushed reciprocal may return as 0.  Checked at |z| in {0, 1, 20, 100}, both signs.
(6) parity: max(1 - cos) <= 1e-3 against the recorded transformers rows, the project's bound for every tower.
    What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
    tests/test_gpu_tower_sharpness.py.
A GPU fault in one test ends the module's GPU work: the tests after it fail without launching anything.
"""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_siglip_text_golden as mk  # noqa: E402
import siglip_text_reference as tr  # noqa: E402
from test_gpu_gemm import BF16, DEV, F32, Guard, assert_bits, assert_close, assert_mutant_far, ulp_bf16  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, SIGLIP_B16, SIGLIP_TEXT_B, CLIPTextGeometry, SiglipTextGeometry, f32_to_bf16_bits,  # noqa: E402
                                               make_clip_text_weights, make_clip_weights, make_siglip_text_weights, make_siglip_weights, round_to_bf16,
                                               siglip_token_ids, synthetic_crops, synthetic_token_ids)

pytestmark = pytest.mark.gpu

I16 = torch.int16
TT = 64
T2 = SiglipTextGeometry(hidden_size=512, num_layers=2, num_heads=8, intermediate_size=2048, vocab_size=256, projection_size=512)  # the quick tower
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


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "siglip_text_cases.npz"))


_weights = {}


def weights_of(key):
    if key not in _weights:
        _weights[key] = make_siglip_text_weights(61, T2) if key == "T2" else make_siglip_text_weights(mk.CASES[key][0], mk.CASES[key][1])
    return _weights[key]


def bf16_dev(x32: np.ndarray):
    """bf16-representable f32 array -> bf16 CUDA tensor"""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV).to(BF16)


# ---------------------------------------------------------------------------------------------------------------------
# (1) token rows at 64 positions


@pytest.mark.parametrize("d, vocab", [(512, 300), (768, 300), (1024, 300), (512, 256000)])
def test_token_rows_64(eng, d, vocab):
    n = 3
    g = torch.Generator(device=DEV).manual_seed(d + vocab)
    tok = torch.randn((vocab, d), generator=g, device=DEV).to(BF16)
    pos = torch.randn((TT, d), generator=g, device=DEV) * 0.7  # f32, not bf16-representable: the sum must round once
    ids = np.random.default_rng(d + vocab).integers(0, vocab, size=(n, TT)).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[2, 63], ids[1, 40] = 0, vocab - 1, vocab - 1, 0  # both ends of the table, the last position
    x = Guard(BF16, n * TT, d)
    eng.siglip_text_apply("token_rows", tok=tok, pos=pos, ids=ids, x=x.view, n=n, d=d, vocab=vocab)
    x.check("token_rows")  # the sentinel rows behind n * 64 (and before row 0) are untouched
    flat = torch.from_numpy(ids.reshape(-1).astype(np.int64)).to(DEV)
    t_of = torch.arange(n * TT, device=DEV) % TT
    want = (tok[flat].float() + pos[t_of]).to(BF16).view(I16)
    assert_bits(x.valid_bits(), want, f"token_rows d {d} vocab {vocab}")
    if vocab <= 300:  # the same in numpy
        tok_h, pos_h = tok.float().cpu().numpy(), pos.cpu().numpy()
        want_h = f32_to_bf16_bits(tok_h[ids.reshape(-1)] + pos_h[np.arange(n * TT) % TT]).astype(np.int16)
        assert np.array_equal(x.valid_bits().cpu().numpy(), want_h)
    # sharpness: 77 positions a sequence (the CLIP layout), and the table row of the neighbouring id
    assert int(((tok[flat].float() + pos[torch.arange(n * TT, device=DEV) % 77 % TT]).to(BF16).view(I16) != want).sum()) > n * TT * d // 4
    assert int(((tok[(flat + 1) % vocab].float() + pos[t_of]).to(BF16).view(I16) != want).sum()) > n * TT * d // 2


# ---------------------------------------------------------------------------------------------------------------------
# (2) attention


def run_attention(eng, qkv32: np.ndarray, n, heads, only_block=-1, out=None, poison=False):
    out = out or Guard(BF16, n * TT, 64 * heads)
    q = bf16_dev(qkv32)
    if poison:  # a NaN row behind the last K / V row: nothing at or past row 64 n may be read
        q = torch.cat([q, torch.full((2, q.shape[1]), float("nan"), dtype=BF16, device=DEV)])[: n * TT]
        assert q.is_contiguous()
    eng.siglip_text_apply("attention", qkv=q, out=out.view, n=n, heads=heads, only_block=only_block)
    out.check(f"attention n {n} heads {heads}")  # canary rows behind row 64 n (and before row 0) untouched
    return out


def check_attention(out, qkv32, n, heads, what):
    ref, A = tr.attention_f64(qkv32, n, heads)
    got = out.valid.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs"
    assert_close(got, torch.from_numpy(ref).to(DEV), torch.from_numpy(tr.attention_tolerance(ref, A)).to(DEV), what)
    return ref, A


@pytest.mark.parametrize("n, heads", [(1, 8), (1, 12), (1, 16), (3, 8), (5, 16), (86, 12), (129, 8), (65, 16)])
def test_attention_against_float64(eng, n, heads):
    qkv = tr.planted_qkv(n, heads, seed=100 + n)
    ref, A = check_attention(run_attention(eng, qkv, n, heads, poison=True), qkv, n, heads, f"attention n {n} heads {heads}")
    if n == 3:  # sharpness: a causal mask, and a softmax over 63 keys, are far outside
        x = np.asarray(qkv, np.float64).reshape(n, TT, 3, heads, 64)
        q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
        s = q @ k.transpose(0, 1, 3, 2)
        tol = torch.from_numpy(tr.attention_tolerance(ref, A))
        for name, keep in (("causal mask", np.tril(np.ones((TT, TT), bool))), ("key 63 dropped", np.arange(TT)[None, :].repeat(TT, 0) < 63)):
            sm = np.where(keep[None, None], s, -np.inf)
            p = np.exp2(sm - sm.max(-1, keepdims=True))
            mut = ((p @ v) / p.sum(-1, keepdims=True)).transpose(0, 2, 1, 3).reshape(n * TT, 64 * heads)
            assert_mutant_far(torch.from_numpy(mut), torch.from_numpy(ref), tol, 64 * heads, name)


@pytest.mark.parametrize("heads", [8, 12, 16])
def test_attention_planted_cases(eng, heads):
    """sequence 0: the dominant key at 0, 31, 32, 63 (heads 0..3), one large finite K row (head 4), a query block whose scores
    are all equal (head 5: Q rows 32..63 zero), an all-zero Q (head 6: the mean of V); sequence 1 as generated"""
    n, D = 2, 64 * heads
    qkv = tr.planted_qkv(n, heads, seed=5).reshape(n, TT, 3, heads, 64)
    u = np.where(np.arange(64) % 3 == 0, -1.0, 1.0).astype(np.float32)
    for h, j in enumerate((0, 31, 32, 63)):
        qkv[0, :, 0, h] += 0.5 * u  # every query leans towards u: 0.5 * 16 * 64 = 512 log2 units for the planted key, a few
        qkv[0, j, 1, h] = 16.0 * u   # for the others: their P is below 2^-149 and leaves as an exact 0
    qkv[0, 40, 1, 4] = 1e30 * u  # scores of +-1e31: one-hot on key 40 for the queries with q . u > 0, weight 0 for the others
    qkv[0, 32:, 0, 5] = 0.0
    qkv[0, :, 0, 6] = 0.0
    qkv = round_to_bf16(qkv).reshape(n * TT, 3 * D)
    assert np.isfinite(qkv).all()
    full = run_attention(eng, qkv, n, heads, poison=True)
    ref, A = check_attention(full, qkv, n, heads, f"planted attention heads {heads}")
    x = qkv.reshape(n, TT, 3, heads, 64)
    got = full.valid.float().cpu().numpy().reshape(n, TT, heads, 64)
    for h, j in enumerate((0, 31, 32, 63)):  # the planted key takes all the weight: the output is its V row, bit for bit
        assert np.array_equal(got[0, :, h], np.broadcast_to(x[0, j, 2, h], (TT, 64))), f"dominant key {j}"
    mean_v = x[0, :, 2, 5].astype(np.float64).mean(0)
    assert np.abs(got[0, 32:, 5] - mean_v).max() <= (2.0 ** -8 * (np.abs(mean_v) + np.abs(x[0, :, 2, 5]).mean(0))).max()
    assert np.array_equal(got[0, 32:, 5], np.broadcast_to(got[0, 32, 5], (32, 64)))  # equal scores: one row for the whole block
    # only_block 0 / 1: the block's rows bit-equal to the full launch, the other block's rows untouched
    for b in (0, 1):
        part = run_attention(eng, qkv, n, heads, only_block=b)
        rows = part.valid_bits().view(n, 2, 32, D)
        assert_bits(rows[:, b].reshape(n * 32, D), full.valid_bits().view(n, 2, 32, D)[:, b].reshape(n * 32, D), f"only_block {b}")
        assert bool((rows[:, 1 - b] == part.sent).all()), f"only_block {b} wrote rows of block {1 - b}"


# ---------------------------------------------------------------------------------------------------------------------
# (3) last-row pool-LN


def ln_ref_np(x, gamma, beta, eps, dtype):
    x, gamma, beta = x.astype(dtype), gamma.astype(dtype), beta.astype(dtype)
    mean = x.mean(1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(eps)) * gamma + beta


@pytest.mark.parametrize("d", [512, 768, 1024])
def test_last_row_pool_ln(eng, d):
    eps, B = 1e-6, 5
    rng = np.random.default_rng(800 + d)
    xh = rng.standard_normal((B * TT, d)).astype(np.float32)
    xh[1 * TT + 63] += 30.0
    xh[2 * TT + 63] *= 100.0
    xh[3 * TT + 63] = 0.0  # a zero row: beta
    gamma = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
    X, G, Bt = torch.from_numpy(xh).to(DEV).to(BF16), torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    y, yf = Guard(BF16, B, d), Guard(F32, B, d)
    eng.siglip_text_apply("last_pool_ln", x=X, gamma=G, beta=Bt, y=y.view, y_f32=yf.view, n=B, d=d, eps=eps)
    y.check("last_pool_ln bf16")
    yf.check("last_pool_ln f32")
    last = X.view(B, TT, d)[:, 63]
    rows = last.float().cpu().numpy()
    e32 = float(np.float32(eps))
    ref = ln_ref_np(rows, gamma, beta, e32, np.float64)
    yard = float(np.abs(ln_ref_np(rows, gamma, beta, e32, np.float32).astype(np.float64) - ref).max())
    floor = max(8 * yard, 2.0 ** -22 * float(np.abs(ref).max()))
    reft = torch.from_numpy(ref).to(DEV)
    tol = ulp_bf16(reft) / 2 + floor
    print(f"last_pool_ln d {d}: float32 yardstick {yard:.3g}")
    assert_close(y.valid.double(), reft, tol, f"last_pool_ln d {d} bf16")
    assert_close(yf.valid.double(), reft, torch.full_like(reft, floor), f"last_pool_ln d {d} f32")
    assert_bits(y.valid_bits(), yf.valid.to(BF16).view(I16), "the bf16 rows are the f32 rows rounded once")
    assert_bits(y.valid[3].view(I16)[None], Bt.to(BF16).view(I16)[None], "zero row: beta")
    # the 77-token instantiation on the same rows (at positions 0, 1, 31, 32, 76 of a CLIP layout): the same bits
    pos77 = np.array([0, 1, 31, 32, 76], dtype=np.int32)
    X77 = torch.zeros((B, 77, d), dtype=BF16, device=DEV)
    X77[torch.arange(B), torch.from_numpy(pos77).long()] = last
    y77 = torch.empty((B, d), dtype=F32, device=DEV)
    eng.text_apply("eos_pool_ln", x=X77.view(B * 77, d), gamma=G, beta=Bt, eos_pos=pos77, y_f32=y77, n=B, d=d, eps=eps)
    assert_bits(yf.valid_bits(), y77.view(torch.int32), "64- and 77-token pool-LN on the same rows")
    other = X.view(B, TT, d)[:, 62].float().cpu().numpy()
    assert_mutant_far(torch.from_numpy(ln_ref_np(other, gamma, beta, e32, np.float64)).to(DEV), reft, tol, B * d // 2, "position 62 pooled")


# ---------------------------------------------------------------------------------------------------------------------
# (4) bias + L2


def l2_ref_np(x, dtype):
    x = x.astype(dtype)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=dtype)), dtype(1e-12))


@pytest.mark.parametrize("P", [64, 256, 512, 1024])
@pytest.mark.parametrize("rows", [1, 5])
def test_bias_l2_rows(eng, rows, P):
    rng = np.random.default_rng(900 + P + rows)
    acc = (rng.standard_normal((rows, P)) * 3.0).astype(np.float32)
    bias = rng.standard_normal(P).astype(np.float32)
    if rows > 1:
        acc[1] *= 1e-3
        acc[2] *= 1e15
        acc[3] = -bias  # y = 0 exactly: a zero row gives zeros
    A, Bv = torch.from_numpy(acc).to(DEV), torch.from_numpy(bias).to(DEV)
    y32, y16 = Guard(F32, rows, P), Guard(BF16, rows, P)
    eng.siglip_text_apply("bias_l2", acc=A, bias=Bv, emb_f32=y32.view, emb_bf16=y16.view, n=rows, p=P)
    y32.check("bias_l2_rows f32")
    y16.check("bias_l2_rows bf16")
    got = y32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(y16.valid_bits(), got.to(BF16).view(I16), "bias_l2_rows: bf16 output vs RNE of the f32 output")
    # y formed once in f32, then l2_rows' arithmetic: the bits of l2_rows on acc + bias
    same = torch.empty((rows, P), dtype=F32, device=DEV)
    eng.clip_apply("l2", xf=(A + Bv[None]).contiguous(), y_f32=same, rows=rows, p=P)
    assert_bits(y32.valid_bits(), same.view(torch.int32), "bias_l2_rows vs l2_rows(acc + bias)")
    yh = acc.astype(np.float64) + bias.astype(np.float64)
    ref = l2_ref_np(yh, np.float64)
    y_f32 = acc + bias
    yard = float(np.abs(l2_ref_np(y_f32, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0 ** -22)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print(f"bias_l2_rows rows {rows} P {P}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    if rows > 1:
        assert bool((got[3] == 0).all()) and bool((y16.valid[3].float() == 0).all())
        assert np.allclose(np.linalg.norm(got.double().cpu().numpy()[[0, 1, 2, 4]], axis=1), 1.0, atol=1e-6)
    nobias = l2_ref_np(acc.astype(np.float64), np.float64)
    keep = [r for r in range(rows) if r not in (2, 3)]  # (row 2 dwarfs the bias, row 3 is the zero row)
    assert int((np.abs(nobias[keep] - ref[keep]) > 4 * tol).sum()) >= len(keep) * P // 2, "mutant 'no bias'"
    only = Guard(BF16, rows, P)
    eng.siglip_text_apply("bias_l2", acc=A, bias=Bv, emb_bf16=only.view, n=rows, p=P)
    assert torch.equal(only.valid_bits(), y16.valid_bits())


# ---------------------------------------------------------------------------------------------------------------------
# (5) scores


def scores_tolerance(c32: np.ndarray, ls: float, lb: float):
    """-> (ref, tol) of the module docstring's bound, float64"""
    s = np.exp(np.float64(np.float32(ls)))
    cs = c32.astype(np.float64) * s
    z = cs + np.float64(np.float32(lb))
    p = tr.sigmoid_f64(z)
    one_minus = tr.sigmoid_f64(-z)
    tol = p * one_minus * (2.0 ** -22 * np.abs(cs) + 2.0 ** -24 * np.abs(z) + 2.0 ** -22) + 2.0 ** -22 * p + 2.0 ** -126
    return p, tol, z


def test_siglip_scores_against_float64(eng):
    ls, lb = float(np.float32(np.log(10.0))), -10.0
    s = np.exp(np.float64(np.float32(ls)))
    zs = np.array([0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0], dtype=np.float64)
    planted = ((zs - lb) / s).astype(np.float32)
    rng = np.random.default_rng(17)
    c = np.concatenate([planted, rng.uniform(-1.0, 1.0, 37 * 1000 - len(planted)).astype(np.float32)]).reshape(37, 1000)
    ref, tol, z = scores_tolerance(c, ls, lb)
    assert np.abs(z.reshape(-1)[: len(zs)] - zs).max() < 1e-5  # the planted |z| in {0, 1, 20, 100}, both signs
    Cd = torch.from_numpy(c).to(DEV)
    out = Guard(F32, 37, 1000)
    eng.siglip_text_apply("scores", cos=Cd, scores=out.view, logit_scale=ls, logit_bias=lb)
    out.check("siglip_scores")
    got = out.valid.double()
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all()) and bool((got <= 1).all())
    assert_close(got, torch.from_numpy(ref).to(DEV), torch.from_numpy(tol).to(DEV), "siglip_scores")
    print("siglip_scores at the planted z:", dict(zip(zs.tolist(), got.view(-1)[: len(zs)].tolist())))
    # the mutants: no bias, a scale that is not exponentiated
    cs = c.astype(np.float64) * s
    for name, mut in (("no bias", tr.sigmoid_f64(cs)), ("scale not exponentiated", tr.sigmoid_f64(c.astype(np.float64) * ls + lb))):
        assert_mutant_far(torch.from_numpy(mut), torch.from_numpy(ref), torch.from_numpy(tol), c.size // 2, name)
    # in place: the same bits; no overflow for large finite inputs of either sign
    inplace = Cd.clone()
    eng.siglip_text_apply("scores", cos=inplace, scores=inplace, logit_scale=ls, logit_bias=lb)
    assert_bits(inplace.view(torch.int32), out.valid_bits(), "in place")
    big = torch.tensor([3e38, -3e38, 1e30, -1e30, 0.0, 88.0, -88.0, 104.0, -104.0], dtype=F32, device=DEV)
    res = torch.empty_like(big)
    eng.siglip_text_apply("scores", cos=big, scores=res, logit_scale=0.0, logit_bias=0.0)
    r = res.cpu().numpy()
    assert np.isfinite(r).all() and r[0] == 1.0 and r[1] == 0.0 and r[2] == 1.0 and r[3] == 0.0 and r[4] == 0.5


# ---------------------------------------------------------------------------------------------------------------------
# (6) the two loaders, and parity with transformers


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_host_and_device_prepared_buffers_are_bit_identical(tmp_path, dtype):
    import test_gpu_weight_prep as wp

    geom = SiglipTextGeometry(hidden_size=512, num_layers=2, num_heads=8, intermediate_size=128, vocab_size=96, projection_size=192)
    ckpt.save_checkpoint(tmp_path, make_siglip_text_weights(21, geom), "siglip_text", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "siglip_text")
    assert ck.dtype == dtype and ck.geometry == geom
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_siglip_text_checkpoint(ck)
        host.load_siglip_text({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (bd, fd), (bh, fh) = wp._read_all(dev), wp._read_all(host)
        info, tg = dev.text_info(), dev.text_geometry()
        assert dev.text_embed_dim == 192 and dev.encoder_info()["kind"] == "vit"  # the image side is untouched
    finally:
        dev.close()
        host.close()
    L = geom.num_layers
    assert info == {"loaded": 1, "hidden_size": 512, "num_layers": L, "num_heads": 8, "intermediate_size": 128, "vocab_size": 96, "projection_dim": 192,
                    "hidden_act": "gelu_pytorch_tanh", "eos_token_id": geom.pad_token_id}
    assert tg == {"kind": "siglip", "tokens": 64, "projection": 192, "pad_token_id": 1}
    assert len(bd) == len(bh) == 4 + 10 * L + 2 and fd == fh
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    # the buffers the tower adds to the CLIP sequence: pos [64, D] and, behind head_w, head_b [P]
    assert bd[1].size * bd[1].itemsize == 64 * 512 * 4 and bd[-1].size * bd[-1].itemsize == 192 * 4 and bd[-2].size * bd[-2].itemsize == 192 * 512 * 2
    hb = np.frombuffer(bd[-1].tobytes(), dtype=np.float32)
    assert np.array_equal(hb, ck.tensors["text_model.head.bias"].float().numpy())


@pytest.mark.parametrize("key", list(mk.CASES))
def test_parity_with_the_recorded_transformers_rows(recorded, key):
    """Measured on one MI355X, max(1 - cos) against transformers: B1 1.3e-5, L2 1.6e-5, S2 1.6e-5, V1 1.3e-5."""
    _, geom, _ = mk.CASES[key]
    ids = recorded[f"{key}.ids"]
    rec = recorded[f"{key}.pooler_output"]
    e = Engine(0)
    try:
        e.load_siglip_text(weights_of(key), geom)
        assert e.text_embed_dim == geom.embed_dim and e.text_geometry()["tokens"] == 64
        e32, e16 = e.text_forward(ids)
        torch.cuda.synchronize()
        if key == mk.WHOLE:  # SiglipModel's logits: sigmoid(logits_per_text) from the engine's own vectors and kernels
            img = torch.from_numpy(recorded[f"{key}.image_embeds"]).to(DEV)
            cos = e.cosine(e16, img.to(BF16).contiguous())
            p = e.siglip_scores(cos).double().cpu().numpy()
    finally:
        e.close()
    got = e32.cpu().numpy()
    assert got.shape == (mk.N_SEQ, geom.embed_dim) and np.isfinite(got).all()
    assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
    omc = tr.one_minus_cos(got, rec)
    print(f"siglip text parity {key}: max(1 - cos) against transformers = {omc.max():.3g} (bound 1e-3), per real length {dict(zip(mk.LENGTHS, np.round(omc, 7)))}")
    assert float(omc.max()) <= 1e-3
    # sharpness: position 62 pooled is far outside the bound.  A head without its bias is NOT told apart by this bound (the
    # seeded bias moves the rows by 5e-4 .. 1.1e-3): test_bias_l2_rows decides that bit for bit, tests/test_siglip_text_cpu.py in float64
    w = weights_of(key)
    wrong = tr.one_minus_cos(tr.siglip_text_embed(ids, w, geom, pool_pos=62), rec)
    print(f"siglip text parity {key}: position 62 pooled: min(1 - cos) = {wrong.min():.3g}")
    assert float(wrong.min()) > 4e-3
    if key == mk.WHOLE:
        # in logit space: a text row within 1 - cos <= 1e-3 of the recorded one is within sqrt(2e-3) of it as a vector, the two
        # bf16 roundings of unit rows add at most 2 * 2^-8, and every unit of cosine is exp(logit_scale) units of logit
        z = np.log(p) - np.log1p(-p)
        bound = float(np.exp(w["logit_scale"][0])) * (np.sqrt(2e-3) + 2.0 ** -7) + 1e-5
        err = float(np.abs(z - recorded[f"{key}.logits_per_text"].astype(np.float64)).max())
        print(f"siglip probabilities {key}: max |logit(p) - recorded logits_per_text| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------------
# (7) coexistence


def _image_rows(e, crops):
    hw = np.tile(np.array([[224, 224]], dtype=np.int32), (crops.shape[0], 1))
    offs = np.arange(crops.shape[0], dtype=np.int64) * (224 * 224 * 3)
    return e.embed(crops.reshape(-1), offs, hw, want_bf16=False)[0]


def test_clip_text_siglip_text_clip_text_on_one_context():
    crops = torch.from_numpy(synthetic_crops(8, seed=3)).to(DEV)
    gc = CLIPTextGeometry(num_layers=2, vocab_size=256, eos_token_id=255)
    wc = make_clip_text_weights(41, gc)
    ids77 = synthetic_token_ids(5, gc.vocab_size, gc.eos_token_id, 13, [2, 20, 33, 64, 77])
    ids64 = siglip_token_ids(5, T2.vocab_size, T2.pad_token_id, 13, [1, 20, 33, 63, 64])
    g_img = dataclasses.replace(CLIP_B16, num_layers=2)
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip(make_clip_weights(15, g_img), g_img)  # a SigLIP text tower under a CLIP image tower: fine at the C level
        before = _image_rows(e, crops).clone()
        n_img = len(e.weights_fingerprint())
        e.load_clip_text(wc, gc)
        fp_clip = e.weights_fingerprint()
        t0 = e.text_forward(ids77, want_bf16=False)[0].clone()
        assert e.text_geometry() == {"kind": "clip", "tokens": 77, "projection": 512, "pad_token_id": 255}
        e.load_siglip_text(weights_of("T2"), T2)
        fp_sig = e.weights_fingerprint()
        assert e.text_geometry()["kind"] == "siglip" and fp_sig[:n_img] == fp_clip[:n_img] and len(fp_sig) == n_img + 4 + 20 + 2
        s0 = e.text_forward(ids64, want_bf16=False)[0].clone()
        ref = tr.siglip_text_embed(ids64, weights_of("T2"), T2)
        assert float(tr.one_minus_cos(s0.cpu().numpy(), ref).max()) <= 1e-3
        with pytest.raises(MmeError, match=r"\[n, 64\]"):
            e.text_forward(ids77)
        assert torch.equal(_image_rows(e, crops).view(torch.int32), before.view(torch.int32))  # image vectors: the same bits
        e.load_clip_text(wc, gc)
        assert e.weights_fingerprint() == fp_clip and e.text_geometry()["kind"] == "clip"
        assert torch.equal(e.text_forward(ids77, want_bf16=False)[0].view(torch.int32), t0.view(torch.int32))  # the first vectors again
        assert torch.equal(_image_rows(e, crops).view(torch.int32), before.view(torch.int32))
        with pytest.raises(MmeError, match="SigLIP text tower"):
            e.siglip_scores(torch.zeros((2, 64), dtype=F32, device=DEV))  # a CLIP text tower has no logit scalars
        # an image reload under a SigLIP text tower leaves the text range alone
        e.load_siglip_text(weights_of("T2"), T2)
        e.load_clip(make_clip_weights(15, g_img), g_img)
        assert torch.equal(e.text_forward(ids64, want_bf16=False)[0].view(torch.int32), s0.view(torch.int32))
    finally:
        e.close()


def test_scores_need_the_two_scalars():
    e = Engine(0)
    try:
        e.load_siglip_text(make_siglip_text_weights(61, T2, logits=None), T2)  # a bare SiglipTextModel
        with pytest.raises(MmeError, match="logit_scale and logit_bias"):
            e.siglip_scores(torch.zeros((2, 64), dtype=F32, device=DEV))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (8) the public interface


def _close_all(emb):
    for e in emb.engines:
        e.close()


def test_region_embedder_siglip_text_tower():
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    g_img = dataclasses.replace(SIGLIP_B16, num_layers=2)
    emb = RegionEmbedder(device=0, encoder="siglip_vit", weights=make_siglip_weights(17, g_img), geometry=g_img, chunk=64, text_tower=True)
    try:
        info = emb.engine.text_info()
        assert (info["hidden_size"], info["num_layers"], info["vocab_size"], info["eos_token_id"]) == (768, 12, 32000, 1)
        assert emb.engine.text_geometry() == {"kind": "siglip", "tokens": 64, "projection": 768, "pad_token_id": 1}
        assert emb.text_embed_dim == emb.embed_dim == 768
        queries = [[5, 6, 7], [9], list(range(100, 164))]
        ids = np.full((3, 64), SIGLIP_TEXT_B.pad_token_id, dtype=np.int32)
        for i, q in enumerate(queries):
            ids[i, : len(q)] = q
        e32, _ = emb.engine.text_forward(ids, want_bf16=False)
        vecs = emb.get_text_embeddings(queries)
        assert np.array_equal(np.array(vecs, dtype=np.float32), e32.cpu().numpy())  # get_text_embeddings == Engine.text_forward
        assert emb.get_text_embeddings([5, 6, 7]) == vecs[0] and emb.get_text_embeddings(ids[1]) == vecs[1]
        with pytest.raises(MmeError, match="65 token ids; supported: at most 64"):
            emb.get_text_embeddings(list(range(65)))
        with pytest.raises(MmeError, match="token ids .* are accepted"):
            emb.get_text_embeddings("a seeded tower brings no tokenizer")
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(24, seed=8)), as_array=True)
        assert ok.all() and rows.shape == (24, 768)
        col = RegionCollection()
        col.upsert(ids=[f"region_{r}" for r in range(24)], embeddings=rows.tolist(),
                   metadatas=[{"parent_image": f"/p/{r // 4}.png", "region_type": "plain_text", "box_str": "0,0,1,1", "area_percentage": 1.0, "is_region": True}
                              for r in range(24)])
        res = col.query(query_texts=queries, embedder=emb, n_results=5, engine=emb.engine)
        # brute force over the stored vectors, in the unit bf16 rows the query ranks
        tq = torch.tensor(vecs, dtype=F32).to(BF16).double().numpy()
        st = torch.from_numpy(rows).to(BF16).double().numpy()
        cos = tq @ st.T
        for i in range(3):  # the five rows a brute-force cosine ranks first (rows closer than 1e-5 to the fifth may swap)
            got_rows = [int(name.split("_")[1]) for name in res["ids"][i]]
            fifth = np.sort(cos[i])[-5]
            assert len(set(got_rows)) == 5 and all(cos[i, r] >= fifth - 1e-5 for r in got_rows), (i, got_rows)
            assert all(cos[i, r] <= fifth + 1e-5 for r in range(24) if r not in got_rows), (i, got_rows)
            assert all(cos[i, a] >= cos[i, b] - 1e-5 for a, b in zip(got_rows, got_rows[1:])), (i, got_rows)
        # probabilities: the float64 formula on the engine's own (bf16) vectors, within the kernel's bound on the f32 cosines
        p = emb.siglip_probabilities(queries, rows)
        assert p.shape == (3, 24) and p.dtype == np.float32
        w = make_siglip_text_weights(emb._seed + 2, SIGLIP_TEXT_B)
        ls, lb = float(w["logit_scale"][0]), float(w["logit_bias"][0])
        tb, ib = torch.tensor(vecs, dtype=F32, device=DEV).to(BF16).contiguous(), torch.from_numpy(rows).to(DEV).to(BF16).contiguous()
        c32 = emb.engine.cosine(tb, ib).cpu().numpy()
        assert np.abs(c32.astype(np.float64) - cos).max() <= 2e-6  # the project's bound for the cosine GEMM
        ref, tol, _ = scores_tolerance(c32, ls, lb)
        assert (np.abs(p.astype(np.float64) - ref) <= tol).all()
        assert np.array_equal(emb.siglip_probabilities(np.array(vecs, dtype=np.float32), rows), p)  # vectors in place of texts
    finally:
        _close_all(emb)


def test_region_embedder_refuses_a_text_tower_of_another_width_and_keeps_the_stub():
    g_img = dataclasses.replace(SIGLIP_B16, num_layers=1)
    wi = make_siglip_weights(17, g_img)
    with pytest.raises(MmeError, match="projection_size = 512; supported: 768"):
        RegionEmbedder(device=0, encoder="siglip_vit", weights=wi, geometry=g_img, chunk=64, text_tower=weights_of("T2"))
    emb = RegionEmbedder(device=0, encoder="siglip_vit", weights=wi, geometry=g_img, chunk=64)  # text_tower=None beside a weight dict
    try:
        with pytest.raises(NotImplementedError):
            emb.get_text_embeddings([1, 2, 3])
        assert emb.engine.text_info()["loaded"] == 0
    finally:
        _close_all(emb)


def test_lazy_load_from_a_whole_siglip_model_directory(tmp_path):
    from test_siglip_text_cpu import _write_whole_model

    g_img = dataclasses.replace(SIGLIP_B16, hidden_size=768, num_layers=1, intermediate_size=256)
    g_txt = dataclasses.replace(T2, intermediate_size=256, projection_size=768)
    tw = make_siglip_text_weights(43, g_txt)
    _write_whole_model(tmp_path / "siglip", tw, g_txt, make_siglip_weights(16, g_img), g_img, torch.bfloat16)
    emb = RegionEmbedder(str(tmp_path / "siglip"), device=0, encoder="siglip_vit", chunk=64)
    try:
        assert emb.embed_dim == 768 and emb.engine.text_info()["loaded"] == 0  # nothing text-side exists before the first call
        n_img = len(emb.engine.weights_fingerprint())
        v = emb.get_text_embeddings([7, 8, 9])
        assert emb.engine.text_geometry()["kind"] == "siglip" and len(v) == 768 and len(emb.engine.weights_fingerprint()) == n_img + 4 + 20 + 2
        row = np.full((1, 64), 1, dtype=np.int64)
        row[0, :3] = [7, 8, 9]
        want = tr.siglip_text_embed(row, tw, g_txt)  # the bf16 file holds the seeded values exactly
        assert float(tr.one_minus_cos(np.array(v, dtype=np.float64)[None], want).max()) <= 1e-3
        p = emb.siglip_probabilities([[7, 8, 9]], np.array(v, dtype=np.float32)[None])  # the directory brought the two scalars
        assert p.shape == (1, 1) and 0.4 < float(p[0, 0]) < 0.6  # cos = 1: sigmoid(10 - 10)
    finally:
        _close_all(emb)


# ---------------------------------------------------------------------------------------------------------------------
# (9) refusals


def test_refusals_leave_the_context_as_it_was():
    e = Engine(0)
    try:
        ids = siglip_token_ids(3, T2.vocab_size, 1, 14, [2, 40, 64])
        e.load_siglip_text(weights_of("T2"), T2)
        good = e.text_forward(ids, want_bf16=False)[0].clone()
        fp = e.weights_fingerprint()
        for change, text in ((dict(max_position_embeddings=77), "max_positions = 77; supported: 64"), (dict(vocab_size=262145), "vocab = 262145; supported: 3..262144"),
                             (dict(hidden_size=1152, num_heads=18), "hidden = 1152; supported: 512, 768, 1024"),
                             (dict(num_heads=12), "heads = 12 at hidden = 512"), (dict(projection_size=96), "projection_size = 96"),
                             (dict(pad_token_id=256), "pad_token_id = 256")):
            g = dataclasses.replace(T2, **change)
            W, layers = Engine._weights_struct("siglip_text", g, lambda name: None, logits=None)  # geometry only: refused before any tensor is read
            assert e.lib.mme_load_siglip_text(e.h, C.byref(W)) != 0 and text in e.lib.mme_last_error(e.h).decode(), change
            assert e.lib.mme_load_siglip_text_as(e.h, C.byref(W), 1, None) != 0 and text in e.lib.mme_last_error(e.h).decode(), change
            assert e.weights_fingerprint() == fp and e.text_geometry()["kind"] == "siglip"
        with pytest.raises(MmeError, match="hidden_act = 'gelu'; supported: gelu_pytorch_tanh"):
            e.load_siglip_text(weights_of("T2"), dataclasses.replace(T2, hidden_act="gelu"))
        assert e.weights_fingerprint() == fp
        oob = ids.copy()
        oob[1, 7] = T2.vocab_size  # an id equal to the vocabulary size
        with pytest.raises(MmeError, match="sequence 1, position 7: id = 256"):
            e.text_forward(oob)
        with pytest.raises(MmeError, match=r"\[n, 64\]"):
            e.text_forward(np.ones((2, 65), dtype=np.int32))  # a 65-id sequence
        assert e.weights_fingerprint() == fp
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(torch.int32), good.view(torch.int32))
        # the one-launch diagnostic refuses what it cannot run
        x = torch.zeros((TT, 512), dtype=BF16, device=DEV)
        f = torch.zeros((TT * 512,), dtype=F32, device=DEV)
        with pytest.raises(MmeError, match="d == 512, d == 768 and d == 1024"):
            e.siglip_text_apply("token_rows", tok=x, pos=f, ids=np.zeros((1, TT)), x=x, n=1, d=384, vocab=TT)
        with pytest.raises(MmeError, match=r"ids_host\[3\] = 64 outside"):
            e.siglip_text_apply("token_rows", tok=x, pos=f, ids=np.array([[0, 1, 2, 64] + [0] * 60]), x=x, n=1, d=512, vocab=TT)
        with pytest.raises(MmeError, match="heads == 8, 12 and 16"):
            e.siglip_text_apply("attention", qkv=x, out=x, n=1, heads=6)
        with pytest.raises(MmeError, match="only_block = 2 outside -1..1"):
            e.siglip_text_apply("attention", qkv=x, out=x, n=1, heads=8, only_block=2)
        with pytest.raises(MmeError, match="p = 96"):
            e.siglip_text_apply("bias_l2", acc=f, bias=f, emb_f32=f, n=1, p=96)
        with pytest.raises(MmeError, match="op 7 outside 0..4"):
            e.siglip_text_apply(7, n=1)
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(torch.int32), good.view(torch.int32))
    finally:
        e.close()
