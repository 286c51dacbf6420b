"""Patch-32 image towers on the GPU (ViT/32 @224: 49 patches of 32 x 32, 50 tokens): the kernels the geometry adds, one
launch at a time (mme_vit32_apply); the prepared weight buffers; the whole pass against the float32 restatement of
tests/clip_reference.py, the rows transformers itself returned (tests/golden/clip32_cases.npz) and oracle.vit; bit
identities; coexistence with patch-16 towers and the text tower on one context; refusals.

(1) retile_patches_p32 and embed_rows_t50 are held BIT FOR BIT: the first is a copy (the numpy mapping of
    tests/test_vit32_cpu.py), the second two IEEE f32 additions in a stated order and one round-to-nearest-even.
(2) attn_fwd_t50 against the float64 pass of tests/test_gpu_attention.py's definition, restated here for 50 tokens: per
    (crop, head) s = q . k (Q carries dh^-0.5 log2 e), p = 2^(s - rowmax), out = sum p v / sum p.  Every input is a bf16
    value and every output element is compared with that file's bound |got - ref| <= 2^-8 |ref| + 2^-8 A,
    A = sum p |v| / sum p: the kernel keeps attention.hip's two rounding points (P to bf16, the output to bf16), each 2^-9
    relative, so 2^-9 (A + 2 |ref|) bounds an exact kernel and 2^-8 (|ref| + A) covers it with a little room.
(3) the 50-token pool forms against float64 with the tolerances tests/test_gpu_clip.py and tests/test_gpu_gemm.py state
    for the 197-token forms: 8 x the deviation of a float32 numpy restatement measured in the test, never below 2^-22 of
    the largest value, plus ulp_bf16(ref) / 2 where the kernel writes bf16.
(4) end to end: max(1 - cos) <= 1e-3, the project's standing bound for the bf16 path.  Measured values: DESIGN.md 4.10.
    What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
    tests/test_gpu_tower_sharpness.py.
"""
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import clip_reference as cr  # noqa: E402
import make_clip32_golden as mk32  # noqa: E402
from test_gpu_clip import _as_vit_names, _golden_crops, _pack, _uniform, l2_ref_np, ln_ref_np  # noqa: E402
from test_gpu_gemm import BF16, DEV, F32, SENT16, Guard, _gen, _randn, assert_bits, assert_close, assert_mutant_bits, assert_mutant_far, ulp_bf16  # noqa: E402
from test_vit32_cpu import retile_np  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, CLIP_B32, VIT_B16, VIT_B32, CLIPGeometry, make_clip_text_weights, make_clip_weights,  # noqa: E402
                                               make_vit_weights, round_to_bf16, synthetic_crops, synthetic_token_ids)

pytestmark = pytest.mark.gpu

I16, I32 = torch.int16, torch.int32
T, NP, DH = 50, 49, 64
CASES = mk32.CASES  # B32: CLIP-B/32; S32: 384 x 2, gelu, P 256; L32n: 1024 x 2, quick_gelu, no projection
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
        _weights[key] = make_clip_weights(*CASES[key])
    return _weights[key]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def crops40():
    return torch.from_numpy(synthetic_crops(40, seed=3)).cuda()


def _close_all(emb):
    for e in emb.engines:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (1) retile_patches_p32, embed_rows_t50


@pytest.mark.parametrize("n", [1, 3, 5])
def test_retile_is_the_mapping_bit_for_bit(eng, n):
    """Element j of run r of the source holds the 16 bits (r + 4099 j) mod 2^16: every 16-element run is unique (r < 47 040)
    and its order shows.  One more crop of sentinel follows the destination: its rows stay as they are."""
    runs = n * 196 * 48
    assert runs < 65536
    bits = ((np.arange(runs, dtype=np.int64)[:, None] + 4099 * np.arange(16)[None, :]) & 0xFFFF).astype(np.uint16).view(np.int16)
    assert np.unique(bits[:, 0]).size == runs  # the first element alone tells the runs apart
    src = torch.from_numpy(bits.reshape(n * 196, 768)).to(DEV)
    dst = Guard(BF16, n * NP, 3072, guard=NP)  # guard = one whole crop of sentinel rows on either side
    eng.vit32_apply("retile", src=src.view(BF16), dst=dst.view, n=n)
    dst.check(f"retile n {n}: the rows of the crops before and after")
    want = torch.from_numpy(retile_np(bits.reshape(n * 196, 768))).to(DEV)
    assert_bits(dst.valid_bits(), want, f"retile n {n}")
    assert_mutant_bits(torch.from_numpy(bits.reshape(n * NP, 3072)).to(DEV), want, n * NP * 3072 // 2, "no permutation")


@pytest.mark.parametrize("rule", ["fit_pad", "clip"])
def test_preprocess_writes_the_retiled_patch16_matrix(rule):
    """Through mme_preprocess on crops of many sizes, under both resize rules: what a patch-32 context emits is the mapping
    applied to what a patch-16 context emits for the same crops, so every guarantee of K1 carries over bit for bit."""
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(224, 224, 3), (40, 300, 3), (700, 90, 3), (224, 100, 3), (333, 512, 3), (17, 19, 3), (1000, 1200, 3)]]
    pix, offs, hw = _pack(arrays)
    g32 = dataclasses.replace(VIT_B32, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=64)
    e16, e32 = Engine(0), Engine(0)
    try:
        e32.load_vit(make_vit_weights(2, g32), geom=g32)
        assert e32.vit_geometry().patch_size == 32 and e16.vit_geometry().patch_size == 16
        for e in (e16, e32):
            e.set_resize_rule(rule)
            e.set_chunk(4)  # two chunks: the staging buffer is reused
        p16 = e16.preprocess(pix, offs, hw)
        p32 = e32.preprocess(pix, offs, hw)
        torch.cuda.synchronize()
        assert tuple(p16.shape) == (7 * 196, 768) and tuple(p32.shape) == (7 * NP, 3072)
        want = retile_np(p16.view(I16).cpu().numpy())
        assert np.array_equal(p32.view(I16).cpu().numpy(), want)
        assert not np.array_equal(p32.view(I16).cpu().numpy().reshape(-1), p16.view(I16).cpu().numpy().reshape(-1))
    finally:
        e16.close()
        e32.close()


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [384, 768, 1024])
def test_embed_rows_t50_bit_for_bit(eng, d, n):
    g = _gen(70 + d + n)
    acc, bias = _randn((n * NP, d), g, 3.0), _randn((d,), g)
    pos, cls = _randn((T, d), g), _randn((d,), g)
    x = Guard(BF16, n * T, d)
    eng.vit32_apply("embed_rows", acc=acc, bias=bias, pos=pos, cls=cls, x=x.view, n=n, d=d)
    x.check("embed_rows_t50")
    a, b, p, c = (t.cpu().numpy() for t in (acc, bias, pos, cls))
    want32 = np.empty((n, T, d), dtype=np.float32)
    want32[:, 1:] = (a.reshape(n, NP, d) + b[None, None]) + p[None, 1:]  # numpy float32: (acc + bias) + pos, IEEE additions
    want32[:, 0] = c + p[0]
    want = torch.from_numpy(want32.reshape(n * T, d)).to(DEV).to(BF16).view(I16)  # round to nearest even
    rows = x.valid_bits()
    clsr = torch.arange(n, device=DEV) * T
    assert_bits(rows[clsr], want[clsr], f"embed_rows_t50 d {d} n {n}: the [CLS] rows")
    assert_bits(rows, want, f"embed_rows_t50 d {d} n {n}")
    mut = want32.copy()
    mut[:, 1:] = (a.reshape(n, NP, d) + b[None, None]) + p[None, :-1]  # the position row of the patch before
    assert_mutant_bits(torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16), want, n * NP * d // 2, "pos[p] for pos[1 + p]")
    mut = want32.copy()
    mut[:, 0] = c + p[1]
    assert_mutant_bits(torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16), want, n * d // 2, "pos[1] for pos[0]")


# ---------------------------------------------------------------------------------------------------------------------
# (2) attention


def _random_qkv(n, H, seed, q_scale=0.25):
    g = _gen(seed)
    x = torch.empty((n * T, 3, H * DH), dtype=BF16, device=DEV)
    x[:, 0] = _randn((n * T, H * DH), g, q_scale, BF16)
    x[:, 1] = _randn((n * T, H * DH), g, 1.0, BF16)
    x[:, 2] = _randn((n * T, H * DH), g, 1.0, BF16)
    return x.view(n * T, 3 * H * DH)


def _view(qkv, H):
    return qkv.view(-1, T, 3, H, DH)


def reference(qkv, H, mutant=None):
    """float64 (out, A), each [n, T, H, dh]; mutant(s [n, H, T, T]) -> scores replaces the true scores (a named kernel bug)"""
    x = _view(qkv, H).double()
    q, k, v = (x[:, :, j].permute(0, 2, 1, 3) for j in range(3))  # [n, H, T, dh]
    s = q @ k.transpose(-1, -2)
    if mutant:
        s = mutant(s)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p @ v) / l).permute(0, 2, 1, 3), ((p @ v.abs()) / l).permute(0, 2, 1, 3)


def _tol(ref, A):
    return 2.0**-8 * (ref.abs() + A)


def attend(eng, qkv, H, only_block=-1, out=None):
    n = qkv.shape[0] // T
    if out is None:
        buf = Guard(BF16, n * T, H * DH)
        eng.vit32_apply("attention", qkv=qkv, out=buf.view, n=n, heads=H, only_block=only_block)
        buf.check("attn_fwd_t50")
        return buf.valid.clone()
    eng.vit32_apply("attention", qkv=qkv, out=out, n=n, heads=H, only_block=only_block)
    return out


def check_close(got, ref, A, H, what):
    g = got.view(-1, T, H, DH).double()
    assert_close(g, ref, _tol(ref, A), what)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_random(eng, H, n):
    qkv = _random_qkv(n, H, 100 + 7 * H + n)
    ref, A = reference(qkv, H)
    check_close(attend(eng, qkv, H), ref, A, H, f"attn_fwd_t50 random H {H} n {n}")


def test_attention_crosses_the_persistent_stride(eng):
    """90 crops x 12 heads = 1080 items on a grid of 1024 workgroups: 56 workgroups take a second item."""
    qkv = _random_qkv(90, 12, 5)
    ref, A = reference(qkv, 12)
    check_close(attend(eng, qkv, 12), ref, A, 12, "attn_fwd_t50 n 90")


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_zero_queries_average_exactly_the_fifty_value_rows(eng, H):
    """Q = 0: every score is 0 and the output is the mean of the crop's own 50 V rows.  LDS rows 50..63 hold clamped copies
    of row 49: counted as keys they would weigh V[49] fifteen times.  In the second launch the first 14 K and V rows of
    crop 1 are huge (1e30): read unclamped and counted, they would drown crop 0's rows."""
    n = 2
    qkv = _random_qkv(n, H, 300 + H)
    x = _view(qkv, H)
    x[:, :, 0] = 0.0
    for huge in (False, True):
        if huge:
            x[1, :14, 1] = 1e30
            x[1, :14, 2] = 1e30
        ref, A = reference(qkv, H)
        mean = x[:, :, 2].double().mean(1, keepdim=True).expand(n, T, H, DH)
        assert bool(((ref - mean).abs() <= 1e-12 * A).all())  # the reference IS the mean
        got = attend(eng, qkv, H)
        check_close(got, ref, A, H, f"attn_fwd_t50 Q = 0, H {H}, huge next crop {huge}")
        tol = _tol(ref, A)
        v = x[:, :, 2].double()
        counted = ((v.sum(1, keepdim=True) + 14 * v[:, 49:50]) / 64).expand(n, T, H, DH)  # the clamped copies as keys
        assert_mutant_far(counted[0], ref[0], tol[0], T * H * DH // 2, "padding rows counted as keys")
        if huge:
            spill = ((v[0].sum(0, keepdim=True) + v[1, :14].sum(0, keepdim=True)) / 64).expand(T, H, DH)  # crop 1's rows 0..13 as keys 50..63
            assert_mutant_far(spill, ref[0], tol[0], T * H * DH // 2, "unclamped reads into the next crop")


SPIKE_KEYS = (0, 31, 32, 49)
SPIKE_ROWS = [0, 31, 32, 49]


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_spikes_at_tile_and_padding_borders(eng, H):
    """Spike keys at the borders of the two 32-key tiles and at the last token (whose clamped copies fill LDS rows 50..63),
    for queries at the borders of the two query blocks; the spike holds most of the row's mass, so both dropping it and
    counting it fifteen times move the output."""
    n = 2
    qkv = _random_qkv(n, H, 400 + H)
    x = _view(qkv, H)
    x[:, :, 1, :, 0] = 0.0  # dim 0 of K: zero except at the spike key
    key_of = torch.tensor([[SPIKE_KEYS[(i * H + h) % 4] for h in range(H)] for i in range(n)], device=DEV)
    for i in range(n):
        for h in range(H):
            x[i, int(key_of[i, h]), 1, h, 0] = 6.0
            x[i, SPIKE_ROWS, 0, h, 0] = 1.0
    ref, A = reference(qkv, H)
    check_close(attend(eng, qkv, H), ref, A, H, f"attn_fwd_t50 spikes H {H}")
    tol = _tol(ref, A)
    onehot = torch.nn.functional.one_hot(key_of, T).bool()[:, :, None, :]  # [n, H, 1, T]

    def dropped(s):
        return s.masked_fill(onehot, float("-inf"))

    def pad_counted(s):  # keys 50..63 are copies of key 49: key 49 weighs 15 x
        s = s.clone()
        s[..., 49] += float(np.log2(15.0))
        return s

    for name, mutant in (("the spike key dropped", dropped), ("padding rows counted as keys", pad_counted)):
        mref, _ = reference(qkv, H, mutant)
        ratio = ((mref - ref).abs() / tol)[:, SPIKE_ROWS].amax(-1)  # [n, rows, H]
        sel = ratio if mutant is dropped else ratio.permute(0, 2, 1)[key_of == 49]
        assert sel.numel() and bool((sel >= 4).all()), f"mutant '{name}' is not separated: {sel.min()}"


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_huge_last_key(eng, H):
    """K row 49 is huge and finite (|k| = 1e30, scores of ~1e30 in either sign, finite in f32); its clamped copies in LDS rows
    50..63 carry the same scores and are removed by selection: nothing but the 50 tokens reaches an output."""
    n = 2
    qkv = _random_qkv(n, H, 500 + H)
    x = _view(qkv, H)
    x[:, 49, 1] = torch.where(x[:, 49, 1] > 0, 1e30, -1e30).to(BF16)
    ref, A = reference(qkv, H)
    assert bool(torch.isfinite(ref).all())
    check_close(attend(eng, qkv, H), ref, A, H, f"attn_fwd_t50 huge key 49, H {H}")


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_only_block(eng, H):
    n = 3
    qkv = _random_qkv(n, H, 600 + H)
    full = attend(eng, qkv, H)
    for blk, rows in ((0, slice(0, 32)), (1, slice(32, T))):
        buf = Guard(BF16, n * T, H * DH)
        attend(eng, qkv, H, only_block=blk, out=buf.view)
        buf.check(f"only_block {blk}")
        got = buf.valid_bits().view(n, T, H * DH)
        assert_bits(got[:, rows].reshape(-1, H * DH), full.view(I16).view(n, T, H * DH)[:, rows].reshape(-1, H * DH), f"only_block {blk}: the computed block")
        other = torch.ones(T, dtype=torch.bool, device=DEV)
        other[rows] = False
        assert bool((got[:, other] == SENT16).all()), f"only_block {blk}: the other block's rows were written"


# ---------------------------------------------------------------------------------------------------------------------
# (3) pool forms


def _pool_inputs(B, tok, d):
    rng = np.random.default_rng(900 + d + tok + B)
    xh = rng.standard_normal((B * T, d)).astype(np.float32)
    if B > 1:
        xh[1 * T + tok] += 30.0
        xh[2 * T + tok] *= 100.0
        xh[3 * T + tok] = 0.0  # zero row: beta
    gamma = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return torch.from_numpy(xh).to(DEV).to(BF16), gamma, beta


@pytest.mark.parametrize("d", [384, 768, 1024])
@pytest.mark.parametrize("tok", [0, 49])
@pytest.mark.parametrize("B", [1, 5])
def test_pool_ln_rows_t50(eng, B, tok, d):
    eps = 1e-5
    X, gamma, beta = _pool_inputs(B, tok, d)
    y = Guard(BF16, B, d)
    eng.vit32_apply("pool_ln", x=X, gamma=torch.from_numpy(gamma).to(DEV), beta=torch.from_numpy(beta).to(DEV), y=y.view, n=B, tok=tok, d=d, eps=eps)
    y.check("pool_ln_rows (50)")
    rows = X.view(B, T, d)[:, tok].float().cpu().numpy()
    e32 = float(np.float32(eps))
    ref = ln_ref_np(rows, gamma, beta, e32, np.float64)
    yard = float(np.abs(ln_ref_np(rows, gamma, beta, e32, np.float32).astype(np.float64) - ref).max())
    floor = max(8 * yard, 2.0**-22 * float(np.abs(ref).max()))
    reft = torch.from_numpy(ref).to(DEV)
    tol = ulp_bf16(reft) / 2 + floor
    assert_close(y.valid.double(), reft, tol, f"pool_ln_rows (50) B {B} tok {tok} d {d}")
    if B > 1:
        assert_bits(y.valid[3].view(I16)[None], torch.from_numpy(beta).to(DEV).to(BF16).view(I16)[None], "zero row: beta")
    other = X.view(B, T, d)[:, tok - 1 if tok else 1].float().cpu().numpy()
    assert_mutant_far(torch.from_numpy(ln_ref_np(other, gamma, beta, e32, np.float64)).to(DEV), reft, tol, B * d // 2, "the neighbouring token pooled")
    if B > 1:  # the 197-token pitch: another row for every crop but the first
        far = X.view(-1, d)[(torch.arange(B, device=DEV) * 197 + tok) % (B * T)].float().cpu().numpy()
        assert_mutant_far(torch.from_numpy(ln_ref_np(far, gamma, beta, e32, np.float64)).to(DEV)[1:], reft[1:], tol[1:], (B - 1) * d // 2, "row b * 197 + tok")


@pytest.mark.parametrize("d", [384, 768, 1024])
@pytest.mark.parametrize("tok", [0, 49])
@pytest.mark.parametrize("B", [1, 5])
def test_pool_ln_l2_t50(eng, B, tok, d):
    eps = 1e-12
    X, gamma, beta = _pool_inputs(B, tok, d)
    gm, bt = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    o32, o16 = Guard(F32, B, d), Guard(BF16, B, d)
    eng.vit32_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, n=B, tok=tok, d=d, eps=eps, emb_f32=o32.view, emb_bf16=o16.view)
    o32.check("pool_ln_l2 (50) f32")
    o16.check("pool_ln_l2 (50) bf16")
    got = o32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(o16.valid_bits(), got.to(BF16).view(I16), "pool_ln_l2 (50): bf16 output vs RNE of the f32 output")
    rows = X.view(B, T, d)[:, tok].float().cpu().numpy()
    e32 = float(np.float32(eps))

    def pool_ref(r, dtype):
        return l2_ref_np(ln_ref_np(r, gamma, beta, e32, dtype), dtype)

    ref = pool_ref(rows, np.float64)
    yard = float(np.abs(pool_ref(rows, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print(f"pool_ln_l2 (50) B {B} tok {tok} d {d}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    other = X.view(B, T, d)[:, tok - 1 if tok else 1].float().cpu().numpy()
    assert int((np.abs(pool_ref(other, np.float64) - ref) > 4 * tol).sum()) >= B * d // 2, "mutant 'neighbouring token' not separated"
    only = Guard(BF16, B, d)
    eng.vit32_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, n=B, tok=tok, d=d, eps=eps, emb_bf16=only.view)
    assert torch.equal(only.valid_bits(), o16.valid_bits())


# ---------------------------------------------------------------------------------------------------------------------
# (4) prepared buffers


def test_prepared_buffers_at_patch_32(tmp_path):
    import test_gpu_weight_prep as wp

    dtype = "bfloat16"
    geom = CLIPGeometry(patch_size=32, hidden_size=384, num_layers=2, num_heads=6, intermediate_size=128, projection_dim=192, hidden_act="gelu")
    ckpt.save_checkpoint(tmp_path, make_clip_weights(21, geom), "clip", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.dtype == dtype and ck.geometry == geom
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_clip_checkpoint(ck)
        host.load_clip({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (bd, fd), (bh, fh) = wp._read_all(dev), wp._read_all(host)
        assert dev.vit_geometry().patch_size == 32 and dev.vit_geometry().seq_len == 50
    finally:
        dev.close()
        host.close()
    D, L = geom.hidden_size, geom.num_layers
    assert len(bd) == len(bh) == 6 + 18 * L + 3 and fd == fh
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    assert bd[1].size == 4 * T * D and bd[5].size == 2 * D * 3072  # pos f32 [50, D], patch_w bf16 [D, 3072]: mme_weights_read order unchanged
    wp.DEV_OF[0] = DEV
    m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    table = wp.vit_table(_as_vit_names(m, geom), geom)
    assert table[2][0] == "patch_b"
    table[2] = ("patch_b", "zeros", D)
    table += [("pre_g", "f32", m["vision_model.pre_layrnorm.weight"]), ("pre_b", "f32", m["vision_model.pre_layrnorm.bias"]),
              ("proj_w", "bf16", m["visual_projection.weight"])]
    folds = wp.check_table(table, bd, "clip patch 32")
    assert len(folds) == 2 * L


# ---------------------------------------------------------------------------------------------------------------------
# (5) end to end


@pytest.mark.parametrize("key", ["B32", "S32", "L32n"])
def test_end_to_end_against_the_restatement_and_transformers(golden_dir, key):
    from oracle import preprocess as opre

    seed, geom = CASES[key]
    w = weights_of(key)
    arrays = list(synthetic_crops(mk32.N_CROPS, seed=0)) + _golden_crops(golden_dir)
    assert len(arrays) == 40
    pv = np.stack([opre.preprocess_crop(a) for a in arrays]).astype(np.float32)
    emb = RegionEmbedder(device=0, encoder="clip", weights=w, geometry=geom, pool="cls", chunk=64)
    try:
        assert emb.embed_dim == geom.embed_dim and emb.engine.vit_geometry().patch_size == 32
        pix, offs, hw = _pack(arrays)
        e32, e16 = emb.embed_packed(pix, offs, hw)
        torch.cuda.synchronize()
        assert emb.engine.attention_redone(geom.num_layers) == [0] * geom.num_layers
        got = e32.cpu().numpy()
        assert got.shape == (40, geom.embed_dim) and np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)
        assert rows.shape == (3, geom.embed_dim) and ok.all() and np.array_equal(rows, got[:3])
    finally:
        _close_all(emb)
    want = cr.clip_embed(pv, w, geom, torch.float32, "cls")
    omc = cr.one_minus_cos(got, want)
    print(f"clip/32 parity {key} ({geom.hidden_size}-d x {geom.num_layers} layers, {geom.hidden_act}, P {geom.projection_dim}): "
          f"max(1 - cos) = {omc.max():.3g} (synthetic 224^2: {omc[:16].max():.3g}, bundled: {omc[16:].max():.3g})")
    assert float(omc.max()) <= 1e-3, (key, float(omc.max()))
    mu = want.mean(axis=0, keepdims=True)
    a, b = got - mu, want - mu  # centred: near-identical seeded-weight embeddings cannot pass trivially
    ccos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert np.all(ccos > 0.98), (key, float(ccos.min()))
    rec = np.load(os.path.join(golden_dir, "clip32_cases.npz"))[f"{key}.image_embeds" if geom.projection_dim else f"{key}.pooler_output"]
    omc_hf = cr.one_minus_cos(got[:16], rec)
    print(f"clip/32 parity {key}: against the recorded transformers rows max(1 - cos) = {omc_hf.max():.3g}")
    assert float(omc_hf.max()) <= 1e-3, (key, float(omc_hf.max()))


@pytest.mark.parametrize("pool", ["cls", "last"])
def test_vit_patch_32_against_the_oracle(golden_dir, pool):
    from oracle import preprocess as opre
    from oracle import vit as ovit

    geom = dataclasses.replace(VIT_B32, num_layers=3)
    w = make_vit_weights(31, geom)
    arrays = list(synthetic_crops(8, seed=2)) + _golden_crops(golden_dir)[:8]
    patches = np.stack([opre.patchify(opre.preprocess_crop(a), 32) for a in arrays])
    assert patches.shape == (16, NP, 3072)
    emb = RegionEmbedder(device=0, encoder="vit", weights=w, geometry=geom, pool=pool, chunk=64)
    try:
        assert emb.embed_dim == 768 and emb.pool_token == (0 if pool == "cls" else 49)
        pix, offs, hw = _pack(arrays)
        got = emb.embed_packed(pix, offs, hw)[0].cpu().numpy()
    finally:
        _close_all(emb)
    want = ovit.vit_embed(patches, w, geom, pool=pool)
    omc = cr.one_minus_cos(got, want)
    print(f"vit/32 parity, pool {pool}: max(1 - cos) = {omc.max():.3g}")
    assert float(omc.max()) <= 1e-3


def test_region_embedder_seeded_geometries_report_512():
    for kw in (dict(encoder="clip", geometry=CLIP_B32),):
        emb = RegionEmbedder(device=0, chunk=64, **kw)
        try:
            assert emb.embed_dim == 512 and emb.engine.vit_geometry().patch_size == 32
            rows, ok = emb.get_image_embeddings(list(synthetic_crops(2, seed=8)), as_array=True)
            assert ok.all() and rows.shape == (2, 512)
        finally:
            _close_all(emb)
    emb = RegionEmbedder(device=0, chunk=64, encoder="vit", geometry=VIT_B32)
    try:
        assert emb.embed_dim == 768 and emb.engine.vit_geometry() == dataclasses.replace(VIT_B32)
    finally:
        _close_all(emb)


# ---------------------------------------------------------------------------------------------------------------------
# (6) bit identities


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_checkpoint_directory_equals_weights_dict(tmp_path, crops40, dtype):
    geom, w = CASES["S32"][1], weights_of("S32")
    ckpt.save_checkpoint(tmp_path, w, "clip", dtype, geometry=geom, image_mean=(0.5, 0.5, 0.5), image_std=(0.25, 0.25, 0.25),
                         image_processor_type="CLIPImageProcessor")
    by_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="clip")
    ck = by_dir.checkpoint
    by_dict = RegionEmbedder(device=0, chunk=64, encoder="clip", weights={k: t.float().numpy() for k, t in ck.tensors.items()}, geometry=geom)
    try:
        by_dict.engine.set_normalisation((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
        assert ck.geometry == geom and ck.dtype == dtype and by_dir.embed_dim == by_dict.embed_dim == 256
        assert by_dir.engine.weights_fingerprint() == by_dict.engine.weights_fingerprint()
        a32, a16 = by_dir.embed_uniform(crops40)
        b32, b16 = by_dict.embed_uniform(crops40)
        torch.cuda.synchronize()
        assert torch.equal(a32, b32) and torch.equal(a16, b16) and bool(torch.isfinite(a32).all()) and tuple(a32.shape) == (40, 256)
    finally:
        _close_all(by_dir)
        _close_all(by_dict)


@pytest.mark.parametrize("key", ["S32", "L32n", "V32"])
def test_forward_settings_are_bit_identical(crops40, key):
    """As the patch-16 test of this name: ln_mode 1 = 2, every GEMM variant, pruned = unpruned, chunking, tile order.  V32 is a
    plain ViT (no pre-LN: the first LayerNorm's statistics come from the canonical pass over x in both folded modes)."""
    eng = Engine(0)
    try:
        if key == "V32":
            geom = dataclasses.replace(VIT_B32, num_layers=2)
            eng.load_vit(make_vit_weights(9, geom), geom=geom)
            width = 768
        else:
            geom = CASES[key][1]
            eng.load_clip(weights_of(key), geom)
            width = geom.embed_dim
        crops = torch.cat([crops40, torch.from_numpy(synthetic_crops(260, seed=9)).cuda()])  # 300 crops = 15 000 rows: interior 256-row tiles and a ragged one
        eng.set_chunk(300)
        eng.set_ln_fusion(1)
        ref, _ = _uniform(eng, crops)
        assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (300, width)
        for variant in (0, 1, 3, 4, 6):
            eng.set_gemm_variant(variant)
            for mode in (2, 1):
                eng.set_ln_fusion(mode)
                got, _ = _uniform(eng, crops)
                assert torch.equal(ref, got), (key, "gemm variant", variant, "ln fusion", mode)
        eng.set_gemm_variant(0)
        eng.set_ln_fusion(2)
        for tok in (0, 31, 32, 49):
            eng.set_forward_pruning(False)
            full, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(True)
            pruned, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(False)
            assert torch.equal(full, pruned), (key, "pruning", tok)
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
        for mode in (0, 2, 1):  # the attention mode keeps its value and changes nothing at 50 tokens
            eng.set_attention_mode(mode)
            got, _ = _uniform(eng, crops40)
            assert torch.equal(got, c8) and eng.attention_redone(geom.num_layers) == [0] * geom.num_layers, (key, "attention mode", mode)
    finally:
        eng.close()


def test_layernorm_kernel_mode_against_the_restatement():
    from oracle import preprocess as opre

    geom, w = CASES["S32"][1], weights_of("S32")
    crops = synthetic_crops(16, seed=0)
    pv = np.stack([opre.preprocess_crop(a) for a in crops]).astype(np.float32)
    eng = Engine(0)
    try:
        eng.load_clip(w, geom)
        eng.set_chunk(64)
        eng.set_ln_fusion(0)
        got0 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
    finally:
        eng.close()
    omc0 = cr.one_minus_cos(got0, cr.clip_embed(pv, w, geom, torch.float32, "cls"))
    print(f"clip/32 parity S32, LayerNorm-kernel mode: max(1 - cos) = {omc0.max():.3g}")
    assert float(omc0.max()) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# (7) coexistence on one context


def test_patch_16_then_32_then_16_on_one_context(crops40):
    g16 = dataclasses.replace(CLIP_B16, num_layers=2)
    g32 = dataclasses.replace(CLIP_B32, num_layers=2)
    w16, w32 = make_clip_weights(15, g16), make_clip_weights(16, g32)
    fresh = Engine(0)
    try:
        fresh.load_clip(w32, g32)
        fresh.set_chunk(64)
        solo32 = [t.clone() for t in _uniform(fresh, crops40)]
    finally:
        fresh.close()
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip(w16, g16)
        first = [t.clone() for t in _uniform(e, crops40)]
        fp16 = e.weights_fingerprint()
        p16 = e.preprocess(*_pack(list(synthetic_crops(2, seed=1))))
        assert e.vit_geometry().patch_size == 16 and tuple(p16.shape) == (2 * 196, 768)
        e.load_clip(w32, g32)
        assert e.vit_geometry().patch_size == 32 and e.vit_geometry().seq_len == 50
        second = _uniform(e, crops40)
        assert torch.equal(second[0], solo32[0]) and torch.equal(second[1], solo32[1])
        p32 = e.preprocess(*_pack(list(synthetic_crops(2, seed=1))))
        assert tuple(p32.shape) == (2 * NP, 3072) and np.array_equal(p32.view(I16).cpu().numpy(), retile_np(p16.view(I16).cpu().numpy()))
        # preprocess -> forward equals embed
        sep = e.vit_forward(e.preprocess(*_pack(list(synthetic_crops(40, seed=3)))))
        torch.cuda.synchronize()
        assert torch.equal(sep[0], solo32[0])
        e.load_clip(w16, g16)
        assert e.vit_geometry().patch_size == 16 and e.weights_fingerprint() == fp16
        third = _uniform(e, crops40)
        assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
        assert not torch.equal(first[0], second[0])
    finally:
        e.close()


def test_text_tower_beside_a_patch_32_tower(crops40):
    from test_gpu_clip_text import T2

    ids = synthetic_token_ids(6, T2.vocab_size, T2.eos_token_id, 13, [2, 20, 33, 64, 70, 77])
    tw = make_clip_text_weights(41, T2)
    g32 = dataclasses.replace(CLIP_B32, num_layers=2)
    alone = Engine(0)
    try:
        alone.load_clip_text(tw, T2)
        t0 = alone.text_forward(ids, want_bf16=False)[0].clone()
    finally:
        alone.close()
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip(make_clip_weights(16, g32), g32)
        img0 = _uniform(e, crops40)[0].clone()
        n_img = len(e.weights_fingerprint())
        e.load_clip_text(tw, T2)
        assert len(e.weights_fingerprint()) == n_img + 4 + 10 * T2.num_layers + 1
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32))
        assert torch.equal(_uniform(e, crops40)[0], img0)
        g16 = dataclasses.replace(CLIP_B16, num_layers=1)
        e.load_clip(make_clip_weights(15, g16), g16)  # an image reload frees its own buffers only
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32))
        e.load_clip(make_clip_weights(16, g32), g32)
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(I32), t0.view(I32)) and torch.equal(_uniform(e, crops40)[0], img0)
    finally:
        e.close()


def test_whole_clip_model_directory_at_patch_32_answers_a_text_query(tmp_path):
    """A clip-vit-base-patch32-shaped directory (vision_config.patch_size 32, both towers, projection 512, vocab.json / merges.txt
    beside the weights): image vectors and text vectors share width 512 and RegionCollection.query(query_texts=...) runs."""
    pytest.importorskip("transformers")
    from safetensors.torch import save_file
    from test_clip_text_cpu import toy_tokenizer_files
    from test_gpu_clip_text import T2

    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    g_img = dataclasses.replace(CLIP_B32, num_layers=2)
    g_txt = dataclasses.replace(T2, vocab_size=195, eos_token_id=194)  # the toy vocabulary
    whole = dict(make_clip_weights(16, g_img))
    whole.update(make_clip_text_weights(43, g_txt))
    whole["logit_scale"] = np.float32([2.6592])
    d = tmp_path / "clip32"
    os.makedirs(d)
    cfg = {"model_type": "clip", "projection_dim": 512,
           "text_config": {"vocab_size": g_txt.vocab_size, "hidden_size": 512, "num_hidden_layers": 2, "num_attention_heads": 8, "intermediate_size": 2048,
                           "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": g_txt.eos_token_id},
           "vision_config": {"image_size": 224, "patch_size": 32, "hidden_size": 768, "num_hidden_layers": 2, "num_attention_heads": 12,
                             "intermediate_size": 3072, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}}
    json.dump(cfg, open(d / "config.json", "w"))
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).contiguous() for k, v in whole.items()}, str(d / "model.safetensors"),
              metadata={"format": "pt"})
    toy_tokenizer_files(d)
    emb = RegionEmbedder(str(d), device=0, encoder="clip", chunk=64)
    try:
        assert emb.embed_dim == 512 and emb.checkpoint.geometry == g_img and emb.engine.text_info()["loaded"] == 0
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(24, seed=8)), as_array=True)
        assert ok.all() and rows.shape == (24, 512)
        v = emb.get_text_embeddings("The news")  # loads the text tower lazily, exactly as at patch 16
        assert emb.engine.text_info()["loaded"] == 1 and len(v) == 512 == emb.text_embed_dim
        col = RegionCollection()
        col.upsert(ids=[f"region_{r}" for r in range(24)], embeddings=rows.tolist(),
                   metadatas=[{"parent_image": f"/p/{r // 4}.png", "region_type": "plain_text", "box_str": "0,0,1,1", "area_percentage": 1.0, "is_region": True}
                              for r in range(24)])
        by_text = col.query(query_texts=["The news", "news"], embedder=emb, n_results=5, engine=emb.engine)
        by_vec = col.query(query_embeddings=[emb.get_text_embeddings(t) for t in ["The news", "news"]], n_results=5, engine=emb.engine)
        assert by_text == by_vec and len(by_text["ids"]) == 2 and len(by_text["ids"][0]) == 5
        rows2, _ = emb.get_image_embeddings(list(synthetic_crops(24, seed=8)), as_array=True)  # the image side is untouched by the text load
        assert np.array_equal(rows, rows2)
    finally:
        _close_all(emb)


def test_a_directory_written_by_save_checkpoint_embeds_crops(tmp_path):
    g = dataclasses.replace(CLIP_B32, num_layers=1)
    w = make_clip_weights(18, g)
    ckpt.save_checkpoint(tmp_path, w, "clip", "bfloat16", geometry=g)
    emb = RegionEmbedder(str(tmp_path), device=0, encoder="clip", chunk=64)
    try:
        assert emb.embed_dim == 512 and emb.checkpoint.geometry == g
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(4, seed=8)), as_array=True)
        assert ok.all() and rows.shape == (4, 512) and np.allclose(np.linalg.norm(rows, axis=1), 1.0, atol=1e-5)
    finally:
        _close_all(emb)


# ---------------------------------------------------------------------------------------------------------------------
# (8) refusals


def test_patch_14_is_refused_and_the_previous_weights_stay(crops40):
    geom, w = CASES["S32"][1], weights_of("S32")
    eng = Engine(0)
    try:
        eng.load_clip(w, geom)
        eng.set_chunk(64)
        before = [t.clone() for t in _uniform(eng, crops40)]
        fp = eng.weights_fingerprint()
        keep = []

        def arr(name):
            a = np.ascontiguousarray(w[name], dtype=np.float32)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_float))

        for patch in (14, 8, 64):
            W, layers = eng._weights_struct("clip", geom, arr)
            W.vit.patch_size = patch
            rc = eng.lib.mme_load_clip(eng.h, C.byref(W))
            text = eng.lib.mme_last_error(eng.h).decode()
            assert rc == -1 and f"patch_size = {patch}; supported: 16, 32" in text, (rc, text)
            assert eng.weights_fingerprint() == fp and eng.vit_geometry().patch_size == 32
        W, layers = eng._weights_struct("clip", geom, arr)
        W.vit.image_size = 384
        assert eng.lib.mme_load_clip(eng.h, C.byref(W)) == -1 and "image_size = 384; supported: 224" in eng.lib.mme_last_error(eng.h).decode()
        e32, e16 = _uniform(eng, crops40)
        assert torch.equal(e32, before[0]) and torch.equal(e16, before[1])
        with pytest.raises(MmeError, match="pool_token 50 outside 0..49"):
            _uniform(eng, crops40, 50)
        with pytest.raises(MmeError, match="patch-32 tower"):
            eng.attention(torch.zeros((197, 3 * 384), dtype=BF16, device=DEV), 0)
        e32, _ = _uniform(eng, crops40)
        assert torch.equal(e32, before[0])
    finally:
        eng.close()


def test_vit32_apply_refuses_bad_arguments(crops40):
    geom, w = CASES["S32"][1], weights_of("S32")
    eng = Engine(0)
    try:
        eng.load_clip(w, geom)
        eng.set_chunk(64)
        before = _uniform(eng, crops40)[0].clone()
        fp = eng.weights_fingerprint()
        d, n = 768, 2
        g = _gen(2)
        gamma, beta = _randn((d,), g), _randn((d,), g)
        x = Guard(BF16, n * T + 1, d)
        y = Guard(BF16, n, d)
        acc, pos = _randn((n * NP + 1, d), g), _randn((T, d), g)
        src, dst = Guard(BF16, n * 196 + 1, 768), Guard(BF16, n * NP, 3072)
        qkv, out = _random_qkv(n, 12, 1), Guard(BF16, n * T, 768)
        cases = [
            (dict(op=5, src=src.view, dst=dst.view, n=n), "op 5 outside 0..4"),
            (dict(op=-1, src=src.view, dst=dst.view, n=n), "op -1 outside 0..4"),
            (dict(op=0, src=src.view, dst=dst.view, n=-1), "n = -1 outside"),
            (dict(op=0, src=src.view.reshape(-1)[1:], dst=dst.view, n=n), "src and dst non-null and 16-byte aligned"),
            (dict(op=0, src=src.view, n=n), "src and dst non-null and 16-byte aligned"),
            (dict(op=0, src=dst.view, dst=dst.view, n=n), "src != dst"),
            (dict(op=1, acc=acc, bias=gamma, pos=pos, cls=beta, x=x.view, n=n, d=512), "built for d == 384, d == 768 and d == 1024 (d = 512)"),
            (dict(op=1, acc=acc, bias=gamma, pos=pos, x=x.view, n=n, d=d), "acc, bias, pos, cls, x non-null and 16-byte aligned"),
            (dict(op=1, acc=acc.reshape(-1)[1:], bias=gamma, pos=pos, cls=beta, x=x.view, n=n, d=d), "16-byte aligned"),
            (dict(op=2, qkv=qkv, out=out.view, n=n, heads=8), "built for heads == 6, 12 and 16 (heads = 8)"),
            (dict(op=2, qkv=qkv, out=out.view, n=n, heads=12, only_block=2), "only_block in -1..1"),
            (dict(op=2, qkv=qkv, n=n, heads=12), "qkv and out non-null and 16-byte aligned"),
            (dict(op=3, x=x.view, gamma=gamma, beta=beta, y=y.view, n=n, tok=50, d=d), "0 <= tok <= 49"),
            (dict(op=3, x=x.view, gamma=gamma, beta=beta, y=y.view, n=n, tok=0, d=1280), "(d = 1280)"),
            (dict(op=3, x=x.view, gamma=gamma, beta=beta, n=n, tok=0, d=d), "y non-null and 16-byte aligned"),
            (dict(op=4, x=x.view, gamma=gamma, beta=beta, n=n, tok=0, d=d), "emb_f32 or emb_bf16"),
            (dict(op=4, x=x.view, gamma=gamma, beta=beta, emb_bf16=y.view.reshape(-1)[1:], n=n, tok=0, d=d), "emb_f32 and emb_bf16 16-byte aligned"),
            (dict(op=4, x=x.view, gamma=None, beta=beta, emb_bf16=y.view, n=n, tok=-1, d=d), "x, gamma, beta non-null"),
        ]
        for kw, text in cases:
            op = kw.pop("op")
            with pytest.raises(MmeError) as ei:
                eng.vit32_apply(op, **kw)
            assert "(-1)" in str(ei.value) and text in str(ei.value), (op, text, str(ei.value))
        for buf in (x, y, src, dst, out):
            assert buf.untouched()
        assert eng.weights_fingerprint() == fp and torch.equal(_uniform(eng, crops40)[0], before)
    finally:
        eng.close()
