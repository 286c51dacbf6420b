"""The ViT/16 family on the GPU: a context runs the geometry its weights were loaded with (ViT-S, -B and -L widths).

What is compared with what, and why the bound is what it is:
  1. Oracle parity.  engine.embed against oracle.preprocess -> oracle.vit.vit_embed(..., geom) (f32 on the CPU) on 16
     synthetic crops plus the 24 bundled variable-size crops of tests/test_gpu_parity.py: max(1 - cos) <= 1e-3, the
     project's bound for this comparison (bf16 MFMA path against an f32 oracle; ViT-B/16 measures 4.8e-5), with that
     file's centred check against the trivial pass.  The worst value per geometry is printed (`pytest -s`).
     What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, tanh- for
     erf-GELU) and what holds it: tests/test_gpu_tower_sharpness.py.
  2. Bit equalities, on 3-layer ViT-S and ViT-L: everything that is the same arithmetic in another order of launches,
     tiles or loaders is compared for EQUALITY (checkpoint directory in f32 / bf16 / f16 against the host loader, the
     fingerprints of the prepared buffers, LayerNorm fusion 1 against 2 under every GEMM variant, pruning, the forced
     exact re-run of the attention against mode 0, chunk 64 against 48, encoder="vit" at ViT-B/16 against "vit_b16").
  3. Attention, exact by construction.  One set of per-head Q / K / V blocks, laid out as a 6-, a 12- and a 16-head
     activation: an item's arithmetic does not depend on the head count, so every (crop, head) present in two layouts
     must come out in the same BITS from the two instantiations (modes 0 and 1; every hsplit of every head count;
     only_block 0..6; reverse).  Heads 12..15 have no ViT-B counterpart and are checked against float64 with the bound
     of tests/test_gpu_attention.py: |got - ref| <= 2^-8 (|ref| + A), A = sum p |v| / sum p.
  4. Row kernels (ops 0, 1, 4, 5) at d = 384 and 1024 and the GEMM epilogues at the family's shapes, against float64
     with the formulas and bounds of tests/test_gpu_gemm.py (imported from there, so they cannot drift apart).  GELU on
     random data: |got - ref| <= gelu_tol(ref) + 1.13 d_x, where d_x is that file's accumulation bound on the
     pre-activation and 1.13 > max |gelu'| = 1.1289.  The pooled row's LayerNorm and L2 step are one arithmetic in every
     token layout (197, 50 and the text tower's 77): the same rows through each layout's hook, compared for EQUALITY.
  5. Two contexts of different geometry in one process, called alternately; a second load into a context.
  6. Downstream at d = 1024 and 384: cross_compare within 2e-6 of float64 numpy on the returned bf16 rows (the cosine
     bound of tests/test_gpu_parity.py), region_neighbours decision for decision against the oracle's loop on the
     kernel's own cosines (as tests/test_gpu_neighbours.py).
  7. A load outside the supported set is MME_E_ARG, names the field, and leaves the context serving its weights.
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd._lib import Engine, MmeError
from multimodal_embeddings_amd.embedder import RegionEmbedder
from multimodal_embeddings_amd.weights import VIT_B16, VIT_L16, VIT_S16, ViTGeometry, make_vit_weights, round_to_bf16, synthetic_crops
from test_gpu_gemm import (BF16, DEV, F32, F64, NP, SENT16, T, U, Guard, _gen, _randn, absacc64, acc64, assert_bits, assert_close, assert_mutant_far,
                           canonical_bounds, check_planes, exact_inputs, exact_value, expected_bits, f32_eps, gelu_ref, gelu_tol, launch,
                           ln_rows, pool_ref, run_stats, stats_ref, token_rows, two_pass_bounds, ulp_bf16)

pytestmark = pytest.mark.gpu

SEED = 7
S3 = dataclasses.replace(VIT_S16, num_layers=3)
L3 = dataclasses.replace(VIT_L16, num_layers=3)
GEOMS = {"S": VIT_S16, "L": VIT_L16, "S3": S3, "L3": L3}
_weights = {}


def weights_of(key):
    """Seeded weights of a geometry, generated once per module (full ViT-L takes about a minute on the CPU)."""
    if key not in _weights:
        _weights[key] = make_vit_weights(SEED, GEOMS[key])
    return _weights[key]


def _pack(arrays, device="cuda:0"):
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(arrays), dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(device), offs, hw


def _golden_crops(golden_dir):
    from PIL import Image

    man = json.load(open(os.path.join(golden_dir, "crops_manifest.json")))
    return [np.array(Image.open(os.path.join(golden_dir, "crops", c["file"])).convert("RGB")) for c in man["crops"]]


def _loaded(key):
    e = Engine(0)
    e.load_vit(weights_of(key))
    return e


def _uniform(engine, crops, pool_token=0):
    n = crops.shape[0]
    per = int(np.prod(crops.shape[1:]))
    offs = np.arange(n, dtype=np.int64) * per
    hw = np.tile(np.array([[crops.shape[1], crops.shape[2]]], dtype=np.int32), (n, 1))
    e32, e16 = engine.embed(crops.reshape(-1), offs, hw, pool_token)
    torch.cuda.synchronize()
    return e32, e16


@pytest.fixture(scope="module")
def crops64():
    return torch.from_numpy(synthetic_crops(64, seed=3)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. oracle parity


@pytest.mark.parametrize("key", ["S", "L3", "L"])
def test_oracle_parity(golden_dir, key):
    from oracle import preprocess as opre
    from oracle import vit as ovit

    geom, w = GEOMS[key], weights_of(key)
    arrays = list(synthetic_crops(16, seed=0)) + _golden_crops(golden_dir)
    assert len(arrays) == 40
    patches = np.stack([opre.preprocess_to_patches(a) for a in arrays])
    eng = _loaded(key)
    try:
        g = eng.vit_geometry()
        assert (g.hidden_size, g.num_layers, g.num_heads, g.intermediate_size) == (geom.hidden_size, geom.num_layers, geom.num_heads, geom.intermediate_size)
        assert eng.embed_dim == geom.hidden_size
        pix, offs, hw = _pack(arrays)
        worst = {}
        for pool, token in (("cls", 0), ("last", 196)):
            e32, e16 = eng.embed(pix, offs, hw, pool_token=token)
            torch.cuda.synchronize()
            assert eng.attention_redone(geom.num_layers) == [0] * geom.num_layers
            got = e32.cpu().numpy()
            assert got.shape == (40, geom.hidden_size) and tuple(e16.shape) == (40, geom.hidden_size)
            assert np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
            assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
            want = ovit.vit_embed(patches, w, geom, pool=pool)
            assert want.shape == got.shape and np.allclose(np.linalg.norm(want, axis=1), 1.0, atol=1e-5)
            one_minus_cos = 1.0 - np.sum(got / np.linalg.norm(got, axis=1, keepdims=True) * want, axis=1)
            worst[pool] = float(one_minus_cos.max())
            print(f"oracle parity {key} ({geom.hidden_size}-d x {geom.num_layers} layers) pool {pool}: max(1 - cos) = {worst[pool]:.3g}")
            assert worst[pool] <= 1e-3, (key, pool, worst[pool])
            mu = want.mean(axis=0, keepdims=True)
            a, b = got - mu, want - mu  # centred: near-identical seeded-weight embeddings cannot pass trivially
            ccos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
            assert np.all(ccos > 0.98), (key, pool, float(ccos.min()))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit equalities


def _host_dict(ck):
    return {k: t.float().numpy() for k, t in ck.tensors.items()}


@pytest.mark.parametrize("key", ["S3", "L3"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_checkpoint_directory_equals_host_path(tmp_path, crops64, key, dtype):
    geom, w = GEOMS[key], weights_of(key)
    ckpt.save_checkpoint(tmp_path, w, "vit", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "vit")
    assert ck.geometry == geom and ck.dtype == dtype
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_vit_checkpoint(ck)
        host.load_vit(_host_dict(ck), eps=geom.layer_norm_eps)
        fd, fh = dev.weights_fingerprint(), host.weights_fingerprint()
        count = 6 + 18 * geom.num_layers
        assert len(fd) == len(fh) == count, (len(fd), len(fh), count)
        differ = [i for i, (a, b) in enumerate(zip(fd, fh)) if a != b]
        assert not differ, f"prepared buffers {differ[:20]} of {count} differ between the device and the host path"
    finally:
        dev.close()
        host.close()
    by_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="vit")
    by_dict = RegionEmbedder(device=0, chunk=64, encoder="vit", weights=_host_dict(ck))
    try:
        assert by_dir.embed_dim == by_dict.embed_dim == geom.hidden_size and by_dir.checkpoint is not None
        a32, a16 = by_dir.embed_uniform(crops64)
        b32, b16 = by_dict.embed_uniform(crops64)
        torch.cuda.synchronize()
        assert torch.equal(a32, b32) and torch.equal(a16, b16)
        assert bool(torch.isfinite(a32).all()) and tuple(a32.shape) == (64, geom.hidden_size)
        if dtype != "float16":  # bf16-representable seeded values survive f32 and bf16 files unchanged: the seeded dict gives the same bits
            seeded = RegionEmbedder(device=0, chunk=64, encoder="vit", geometry=geom, seed=SEED)
            c32, _ = seeded.embed_uniform(crops64)
            torch.cuda.synchronize()
            assert torch.equal(a32, c32)
            for e in seeded.engines:
                e.close()
    finally:
        for emb in (by_dir, by_dict):
            for e in emb.engines:
                e.close()


@pytest.mark.parametrize("key", ["S3", "L3"])
def test_forward_settings_are_bit_identical(crops64, key):
    geom = GEOMS[key]
    eng = _loaded(key)
    try:
        eng.set_chunk(64)
        crops = torch.cat([crops64, torch.from_numpy(synthetic_crops(236, seed=9)).cuda()])  # 300 crops: 230 row tiles of 256 + 220 rows
        eng.set_chunk(300)
        eng.set_ln_fusion(1)
        ref, ref16 = _uniform(eng, crops)
        assert bool(torch.isfinite(ref).all())
        for variant in (0, 1, 3, 4, 6):
            eng.set_gemm_variant(variant)
            for mode in (2, 1):
                eng.set_ln_fusion(mode)
                got, _ = _uniform(eng, crops)
                assert torch.equal(ref, got), (key, "gemm variant", variant, "ln fusion", mode)
        eng.set_gemm_variant(0)
        eng.set_ln_fusion(2)
        # pruning on / off, both pooled tokens
        for tok in (0, 196):
            eng.set_forward_pruning(False)
            full, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(True)
            pruned, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(False)
            assert torch.equal(full, pruned), (key, "pruning", tok)
        # the forced exact re-run of every attention launch against the exact form
        eng.set_attention_mode(0)
        exact, _ = _uniform(eng, crops)
        assert eng.attention_redone(geom.num_layers) == [0] * geom.num_layers
        eng.set_attention_mode(2)
        forced, _ = _uniform(eng, crops)
        assert eng.attention_redone(geom.num_layers) == [1] * geom.num_layers
        assert len(eng.attention_redone()) == 12 and eng.attention_redone()[: geom.num_layers] == [1] * geom.num_layers
        eng.set_attention_mode(1)
        assert torch.equal(exact, forced), (key, "attention mode 2 vs 0")
        fast, _ = _uniform(eng, crops)
        assert float((1.0 - (fast * exact).sum(dim=1)).max()) <= 1e-4
        # chunk 64 against chunk 48 (passes of 48 and 16 crops: ragged last row tiles) on the 64 crops
        eng.set_chunk(64)
        c64, _ = _uniform(eng, crops64)
        eng.set_chunk(48)
        c48, _ = _uniform(eng, crops64)
        assert torch.equal(c64, c48), (key, "chunk 64 vs 48")
        assert torch.equal(c64, ref[:64]), (key, "the same crops inside a pass of 300")
        # tile order
        for order in (0, 2, 1):
            eng.set_tile_order(order)
            got, _ = _uniform(eng, crops64)
            assert torch.equal(got, c48), (key, "tile order", order)
    finally:
        eng.close()


def test_encoder_vit_at_vit_b16_equals_vit_b16(crops64):
    a = RegionEmbedder(device=0, chunk=64, encoder="vit", geometry=VIT_B16, seed=SEED)
    b = RegionEmbedder(device=0, chunk=64, encoder="vit_b16", seed=SEED)
    try:
        assert a.embed_dim == b.embed_dim == 768
        a32, a16 = a.embed_uniform(crops64)
        b32, b16 = b.embed_uniform(crops64)
        torch.cuda.synchronize()
        assert torch.equal(a32, b32) and torch.equal(a16, b16)
        assert a.engine.weights_fingerprint() == b.engine.weights_fingerprint()
    finally:
        for emb in (a, b):
            for e in emb.engines:
                e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. attention


@pytest.fixture(scope="module")
def attn_engines():
    """{heads: context whose geometry has that many heads}; 12: a context nothing was loaded into (ViT-B/16)."""
    one_layer = {6: dataclasses.replace(VIT_S16, num_layers=1), 16: dataclasses.replace(VIT_L16, num_layers=1)}
    engines = {12: Engine(0)}
    for h, g in one_layer.items():
        engines[h] = Engine(0)
        engines[h].load_vit(make_vit_weights(SEED, g))
    for h, e in engines.items():
        assert e.vit_geometry().num_heads == h
    yield engines
    for e in engines.values():
        e.close()


def _blocks(n, seed, q_scale=0.25):
    """per-head Q / K / V blocks [n * 197, 3, 16, 64] bf16: Q ~ N(0, q_scale), K, V ~ N(0, 1)"""
    g = _gen(seed)
    x = torch.randn((n * T, 3, 16, 64), generator=g, device=DEV)
    x[:, 0] *= q_scale
    return x.to(BF16)


def _layout(blocks, heads):
    """the [n * 197, 3 * 64 * heads] activation that holds heads 0..heads-1 of the blocks"""
    return blocks[:, :, :heads].contiguous().view(blocks.shape[0], 3 * heads * 64)


def _attend(eng, qkv, mode, **kw):
    eng.set_attention_mode(mode)
    try:
        out = torch.zeros((qkv.shape[0], qkv.shape[1] // 3), dtype=BF16, device=DEV)  # only_block leaves the other rows alone
        out, redone = eng.attention(qkv, 0, out=out, **kw)
    finally:
        eng.set_attention_mode(1)
    return out, redone


def _attention_ref(blocks, heads):
    """float64 (out, A) [n, 197, len(heads), 64] from the definition: s = q . k (base-2 logits), p = 2^(s - max), out = p v / sum p"""
    x = blocks.view(-1, T, 3, 16, 64)[:, :, :, heads].double()
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))  # [n, h, T, 64]
    s = q @ k.transpose(2, 3)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p @ v) / l).transpose(1, 2), ((p @ v.abs()) / l).transpose(1, 2)


# every hsplit of every head count (launch_attention: the smallest divisor d of H with n d >= 512, else H):
# H = 6: 6 (n < 171), 3, 2, 1;  H = 12: 12 (n < 86), 6, 4, 3, 2, 1;  H = 16: 16 (n < 64), 8, 4, 2, 1
@pytest.mark.parametrize("n", [1, 5, 300, 64, 90, 128, 171, 512])
def test_attention_bits_do_not_depend_on_head_count(attn_engines, n):
    blocks = _blocks(n, 4000 + n)
    outs = {}
    for mode in (0, 1):
        for h, eng in attn_engines.items():
            out, redone = _attend(eng, _layout(blocks, h), mode)
            assert not redone, (n, mode, h)
            assert bool(torch.isfinite(out.float()).all())
            outs[mode, h] = out.view(-1, h, 64)
        for h in (6, 16):
            common = min(h, 12)
            same = torch.equal(outs[mode, h][:, :common].contiguous().view(torch.int16), outs[mode, 12][:, :common].contiguous().view(torch.int16))
            assert same, f"n {n} mode {mode}: the {h}-head instantiation differs in bits from the 12-head one on heads 0..{common - 1}"
    if n <= 300:  # heads 12..15 against float64, every head of the 6-head layout too
        for h, heads in ((16, [12, 13, 14, 15]), (6, [0, 1, 2, 3, 4, 5])):
            ref, A = _attention_ref(blocks, heads)
            for mode in (0, 1):
                got = outs[mode, h].view(n, T, h, 64)[:, :, heads].double()
                err, tol = (got - ref).abs(), 2.0**-8 * (ref.abs() + A)
                ratio = float((err / tol).max())
                print(f"attention n {n} H {h} heads {heads[0]}..{heads[-1]} mode {mode}: max err / tol = {ratio:.3g}")
                assert ratio <= 1.0, (n, h, mode, ratio)
                # sharpness: the neighbouring head's output leaves the tolerance almost everywhere
                other = outs[mode, h].view(n, T, h, 64)[:, :, [x - 1 for x in heads]].double()
                assert float(((other - ref).abs() > 4 * tol).double().mean()) > 0.5


def test_attention_only_block_reverse_and_forced_rerun(attn_engines):
    n = 5
    blocks = _blocks(n, 4242)
    full = {h: _attend(eng, _layout(blocks, h), 0)[0] for h, eng in attn_engines.items()}
    for h, eng in attn_engines.items():
        qkv = _layout(blocks, h)
        for mode in (0, 1):
            whole, _ = _attend(eng, qkv, mode)
            rev, _ = _attend(eng, qkv, mode, reverse=True)
            assert torch.equal(rev.view(torch.int16), whole.view(torch.int16)), (h, mode, "reverse")
            for blk in range(7):
                part, _ = _attend(eng, qkv, mode, only_block=blk)
                rows = torch.arange(n * T, device=DEV).view(n, T)[:, 32 * blk : 32 * blk + 32].reshape(-1)
                assert torch.equal(part[rows].view(torch.int16), whole[rows].view(torch.int16)), (h, mode, "only_block", blk)
                rest = torch.ones(n * T, dtype=torch.bool, device=DEV)
                rest[rows] = False
                assert bool((part[rest].view(torch.int16) == 0).all()), (h, mode, "only_block wrote other rows", blk)
                if h != 12:
                    common = min(h, 12)
                    p12, _ = _attend(attn_engines[12], _layout(blocks, 12), mode, only_block=blk, reverse=bool(blk & 1))
                    assert torch.equal(part.view(-1, h, 64)[rows][:, :common].contiguous().view(torch.int16),
                                       p12.view(-1, 12, 64)[rows][:, :common].contiguous().view(torch.int16)), (h, mode, blk)
        forced, redone = _attend(eng, qkv, 2)
        assert redone and torch.equal(forced.view(torch.int16), full[h].view(torch.int16)), (h, "mode 2 vs mode 0")
    bad = torch.zeros((T, 3 * 768), dtype=BF16, device=DEV)
    with pytest.raises(MmeError, match="1152"):  # a 12-head activation handed to the 6-head context
        attn_engines[6].attention(bad, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. row kernels and GEMM epilogues at the new widths


@pytest.mark.parametrize("d", [384, 1024])
def test_two_pass_statistics_and_layernorm_rows(d):
    eng = Engine(0)
    eps = 1e-12
    e32 = f32_eps(eps)
    X, fam = ln_rows(d, 777 + d)
    rows = NP
    mean_ref, var_ref = stats_ref(X)
    d_mean, d_var = two_pass_bounds(X, e32)
    st = run_stats(eng, "ln_stats", rows, x=X, rows=rows, d=d, eps=eps)
    mean, var = st[:, 0].double(), st[:, 1].double() ** -2 - e32
    assert bool(torch.isfinite(st).all())
    print(f"ln_stats_rows d {d}: max err / bound: mean {float(((mean - mean_ref).abs() / d_mean.clamp_min(1e-300)).max()):.3g} "
          f"var {float(((var - var_ref).abs() / d_var).max()):.3g}")
    assert bool(((mean - mean_ref).abs() <= d_mean).all()), "ln_stats_rows: mean outside its bound"
    assert bool(((var - var_ref).abs() <= d_var).all()), "ln_stats_rows: variance outside its bound"
    ro = fam["offset30"]
    assert bool(((((X.double() ** 2).mean(1) - var_ref).abs() > 4 * d_var)[ro]).all()), "mutant 'rstd without - mean^2' is not separated"
    # a ragged last block of four rows, and rows the launch must not touch
    part = run_stats(eng, "ln_stats", rows, x=X, rows=rows - 3, d=d, eps=eps)
    assert torch.equal(part[: rows - 3].view(torch.int32), st[: rows - 3].view(torch.int32)) and bool(torch.isnan(part[rows - 3 :]).all())
    g = _gen(31 + d)
    gamma, beta = (1.0 + _randn((d,), g, 0.2)).contiguous(), _randn((d,), g, 0.5)
    y = Guard(BF16, rows, d)
    eng.rowop_apply("layernorm", x=X, y=y.view, gamma=gamma, beta=beta, rows=rows, d=d, eps=eps)
    y.check("layernorm_rows")
    x = X.double()
    rstd_ref = (var_ref + e32) ** -0.5
    ref = (x - mean_ref[:, None]) * rstd_ref[:, None] * gamma.double() + beta.double()
    e = d * 2.0**-23
    tol = ulp_bf16(ref) / 2 + e * ((x.abs() + mean_ref.abs()[:, None]) * rstd_ref[:, None] * gamma.double().abs() + beta.double().abs())
    assert_close(y.valid.double(), ref, tol, f"layernorm_rows d {d}")
    assert_mutant_far(ref - beta.double(), ref, tol, ref.numel() // 4, "beta dropped")
    keep = torch.cat([fam["normal"], fam["small"], fam["massive"]])
    mg = (x - mean_ref[:, None]) * rstd_ref[:, None] * torch.roll(gamma, 1).double() + beta.double()
    assert_mutant_far(mg[keep], ref[keep], tol[keep], keep.numel() * d // 8, "gamma of the neighbouring column")
    eng.close()


@pytest.mark.parametrize("d", [384, 1024])
@pytest.mark.parametrize("B", [1, 5, 1000])
def test_cls_rows_bit_for_bit(d, B):
    eng = Engine(0)
    g = _gen(60 + B + d)
    cls, pos = _randn((d,), g), _randn((T, d), g)
    x = Guard(BF16, B * T, d)
    eng.rowop_apply("cls_rows", x=x.view, cls=cls, pos=pos, B=B, d=d)
    x.check("cls_rows")
    want = torch.full((B * T, d), SENT16, dtype=torch.int16, device=DEV)
    want[torch.arange(B, device=DEV) * T] = (cls + pos[0]).to(BF16).view(torch.int16)
    assert_bits(x.valid_bits(), want, f"cls_rows d {d} B {B}")
    eng.close()


@pytest.mark.parametrize("d", [384, 1024])
@pytest.mark.parametrize("tok", [0, 77, 196])
def test_pool_ln_l2(d, tok):
    eng = Engine(0)
    B, eps = 37, 1e-12
    rng = np.random.default_rng(500 + tok + d)
    xh = rng.standard_normal((B * T, d)).astype(np.float32)
    xh[(np.arange(B) * T + tok)[5]] += 30.0
    xh[(np.arange(B) * T + tok)[6]] *= 100.0
    xh[(np.arange(B) * T + tok)[7]] = 0.0
    gamma = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(d)).astype(np.float32)
    X = torch.from_numpy(xh).to(DEV).to(BF16)
    gm, bt = torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)
    e32, e16 = Guard(F32, B, d), Guard(BF16, B, d)
    eng.rowop_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, B=B, tok=tok, d=d, eps=eps, emb_f32=e32.view, emb_bf16=e16.view)
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
    print(f"pool_ln_l2 d {d} tok {tok}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, f"pool_ln_l2 d {d} tok {tok}: max deviation {err:.3g} > {tol:.3g}"
    bn = beta.astype(np.float64) / np.linalg.norm(beta.astype(np.float64))
    assert float(np.abs(got[7].double().cpu().numpy() - bn).max()) <= tol, "zero row: output is not beta / ||beta||"
    other = X.view(B, T, d)[:, tok - 1 if tok else 1].float().cpu().numpy()
    assert int((np.abs(pool_ref(other, gamma, beta, eps, np.float64) - ref) > 4 * tol).sum()) >= B * d // 2, "mutant 'neighbouring token' not separated"
    eng.close()


@pytest.mark.parametrize("d", [384, 768, 1024])
@pytest.mark.parametrize("tok", [0, 49])
def test_pooled_row_is_one_arithmetic_in_every_layout(d, tok):
    """The LayerNorm of a pooled row and its L2 step are written once (csrc/row_kernels.h): the same 5 rows at token `tok`
    of a 197-token, a 50-token and (text widths) a 77-token stream must leave every pooling hook in the same BITS."""
    eng = Engine(0)
    B, eps = 5, 1e-5
    g = _gen(900 + d + tok)
    rows = _randn((B, d), g).to(BF16)
    gm, bt = (1.0 + _randn((d,), g, 0.2)).contiguous(), _randn((d,), g, 0.5)

    def stream(tokens):
        x = _randn((B, tokens, d), g).to(BF16)
        x[:, tok] = rows
        return x.view(B * tokens, d).contiguous()

    x197, x50 = stream(T), stream(50)
    a32, a16, b32, b16 = Guard(F32, B, d), Guard(BF16, B, d), Guard(F32, B, d), Guard(BF16, B, d)
    eng.rowop_apply("pool_ln_l2", x=x197, gamma=gm, beta=bt, B=B, tok=tok, d=d, eps=eps, emb_f32=a32.view, emb_bf16=a16.view)
    eng.vit32_apply("pool_ln_l2", x=x50, gamma=gm, beta=bt, n=B, tok=tok, d=d, eps=eps, emb_f32=b32.view, emb_bf16=b16.view)
    for buf in (a32, a16, b32, b16):
        buf.check("pool_ln_l2")
    assert bool(torch.isfinite(a32.valid).all()) and float(a32.valid.abs().max()) > 0
    assert_bits(b32.valid_bits(), a32.valid_bits(), f"pool_ln_l2 f32, 50 against 197 tokens, d {d} tok {tok}")
    assert_bits(b16.valid_bits(), a16.valid_bits(), f"pool_ln_l2 bf16, 50 against 197 tokens, d {d} tok {tok}")
    y197, y50 = Guard(BF16, B, d), Guard(BF16, B, d)
    eng.clip_apply("pool_ln", x=x197, gamma=gm, beta=bt, y=y197.view, B=B, tok=tok, d=d, eps=eps)
    eng.vit32_apply("pool_ln", x=x50, gamma=gm, beta=bt, y=y50.view, n=B, tok=tok, d=d, eps=eps)
    y197.check("pool_ln")
    y50.check("pool_ln")
    assert_bits(y50.valid_bits(), y197.valid_bits(), f"pool_ln, 50 against 197 tokens, d {d} tok {tok}")
    if d != 384:  # 384 is no text width
        y77 = Guard(BF16, B, d)
        eng.text_apply("eos_pool_ln", x=stream(77), gamma=gm, beta=bt, eos_pos=[tok] * B, y=y77.view, n=B, d=d, eps=eps)
        y77.check("eos_pool_ln")
        assert_bits(y77.valid_bits(), y197.valid_bits(), f"eos_pool_ln against pool_ln, d {d} tok {tok}")
    eng.close()


def test_rowops_still_refuse_other_widths():
    eng = Engine(0)
    x = torch.zeros((T, 1280), dtype=BF16, device=DEV)
    st = torch.zeros((T, 2), dtype=F32, device=DEV)
    for d in (64, 512, 1280):
        with pytest.raises(MmeError, match="d == 768"):
            eng.rowop_apply("ln_stats", x=x, stats=st, rows=1, d=d)
    eng.close()


# (epilogue, M, N, K): the family's GEMM shapes with the epilogue the forward runs on them, M with a ragged last row
# tile (600 = 2 x 256 + 88; patch embed 3 crops = 588 rows).  N = 384 and 1152 end in a ragged COLUMN tile, whose outputs
# come from the edge-tile epilogue; that one leaves no partial-sum planes, which is why the forward derives the
# statistics from x at 384 (epilogue 8 is still run there, as tests/test_gpu_gemm.py runs it at N = 320: outputs only).
FAMILY_EXACT = [
    (3, 3 * NP, 384, 768, {"amax": 1}),                    # patch embed, ViT-S (no planes: the forward asks for none at 384)
    (4, 600, 384, 768, {}),
    (0, 600, 384, 768, {}),
    (5, 600, 1152, 384, {}),                               # QKV, LN folded, ViT-S
    (0, 600, 1152, 384, {}),
    (8, 600, 384, 384, {"amax": 1}),                       # o_proj, ViT-S
    (8, 600, 384, 1536, {"amax": 1}),                      # fc2, ViT-S
    (2, 600, 384, 1536, {"inplace": False}),
    (5, 600, 1536, 384, {}),                               # fc1 before its GELU, ViT-S
    (3, 3 * NP, 1024, 768, {"amax": 1, "planes": True}),  # patch embed, ViT-L
    (5, 600, 3072, 1024, {}),                              # QKV, ViT-L
    (8, 600, 1024, 1024, {"amax": 1}),                     # o_proj, ViT-L
    (5, 600, 4096, 1024, {}),                              # fc1, ViT-L
    (8, 600, 1024, 4096, {"amax": 1}),                     # fc2, ViT-L
    (2, 600, 1024, 4096, {}),
    (4, 600, 1024, 4096, {}),
]


@pytest.mark.parametrize("case", FAMILY_EXACT, ids=lambda c: f"epi{c[0]}-M{c[1]}-N{c[2]}-K{c[3]}")
def test_gemm_family_shapes_exact(case):
    eng = Engine(0)
    epi, M, N, K, opt = case
    what = f"exact epilogue {epi} M {M} N {N} K {K}"
    d = exact_inputs(epi, M, N, K, 7000 + 13 * M + N + K + epi, amax=opt.get("amax", 3))
    value = exact_value(epi, d)
    want = expected_bits(epi, d, value, what)
    give_planes = epi == 8 or (epi == 3 and opt.get("planes", False))
    for variant, rev in [(1, 0), (3, 0), (4, 0), (4, 1), (0, 0)]:
        w = f"{what} variant {variant} reverse {rev}"
        out, planes, ran = launch(eng, epi, d["A"], d["W"], variant, reverse_m=rev, bias=d.get("bias"), res=d.get("res"),
                                  inplace=opt.get("inplace", True), pos=d.get("pos"), ln_stats=d.get("ln_stats"), colsum=d.get("colsum"),
                                  planes=give_planes, what=w)
        assert_bits(out.view(torch.int32 if epi == 4 else torch.int16), want, w)
        if give_planes:
            check_planes(epi, planes, want, M, N, ran, w)
    eng.close()


FAMILY_RANDOM = [(3, 3 * NP, 384, 768), (8, 600, 384, 1536), (8, 600, 384, 384), (4, 600, 384, 768), (3, 3 * NP, 1024, 768), (8, 600, 1024, 4096),
                 (8, 600, 1024, 1024), (0, 600, 1152, 384), (0, 600, 3072, 1024)]


@pytest.mark.parametrize("case", FAMILY_RANDOM, ids=lambda c: f"epi{c[0]}-M{c[1]}-N{c[2]}-K{c[3]}")
def test_gemm_family_shapes_random(case):
    eng = Engine(0)
    epi, M, N, K = case
    what = f"random epilogue {epi} M {M} N {N} K {K}"
    g = _gen(9000 + M + N + K + epi)
    A, W = _randn((M, K), g, 1.0, BF16), _randn((N, K), g, 1.0, BF16)
    rows = M // NP * T if epi == 3 else M
    bias = _randn((N,), g) if epi != 4 else None
    res = _randn((rows, N), g, 1.0, BF16) if epi in (2, 8) else None
    pos = _randn((T, N), g) if epi == 3 else None
    acc, aab = acc64(A, W), absacc64(A, W)
    ref, mag = acc.clone(), acc.abs()
    for extra in (bias, res):
        if extra is not None:
            ref += extra.double()
            mag += extra.double().abs()
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
        out, planes, ran = launch(eng, epi, A, W, variant, bias=bias, res=res, pos=pos, planes=epi == 8, what=w)
        if epi == 3:
            cls = out[torch.arange(M // NP, device=DEV) * T].view(torch.int16)
            assert bool((cls == SENT16).all()), f"{w}: a [CLS] row was written"
            out = out[token_rows(M)]
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    bits = torch.int32 if epi == 4 else torch.int16
    for o in outs[1:]:
        assert torch.equal(o.view(bits), outs[0].view(bits)), f"{what}: variants differ in bits"
    if K <= 768:
        assert_mutant_far(ref - acc + acc64(A[:, : K - 64], W[:, : K - 64]), ref, tol, ref.numel() // 2, "last K-tile dropped")
    eng.close()


@pytest.mark.parametrize("epi,M,N,K", [(1, 600, 1536, 384), (6, 600, 1536, 384), (1, 600, 4096, 1024), (6, 600, 4096, 1024)])
def test_gemm_family_shapes_gelu(epi, M, N, K):
    """fc1 of ViT-S and ViT-L: GELU of (acc + bias) on random data, with the LayerNorm fold's algebra (epilogue 6) at a
    planted (mean, rstd).  Bound: module docstring, 4."""
    eng = Engine(0)
    g = _gen(9500 + N + K + epi)
    A, W = _randn((M, K), g, 1.0, BF16), _randn((N, K), g, 1.0 / K**0.5, BF16)  # pre-activations of order 1
    bias = _randn((N,), g)
    acc, aab = acc64(A, W), absacc64(A, W)
    kw = {}
    if epi == 6:
        mean = _randn((M,), g, 0.25)
        rstd = (0.5 + torch.rand((M,), generator=g, device=DEV)).float()
        colsum = _randn((N,), g)
        kw = dict(ln_stats=torch.stack([mean, rstd], 1).contiguous(), colsum=colsum)
        core = acc - mean.double()[:, None] * colsum.double()[None, :]
        x = rstd.double()[:, None] * core + bias.double()
        dx = rstd.double()[:, None] * (K * 2.0**-23 * aab + 4 * U * (acc.abs() + (mean.double()[:, None] * colsum.double()[None, :]).abs())) + 4 * U * x.abs()
    else:
        x = acc + bias.double()
        dx = K * 2.0**-23 * aab + 4 * U * (acc.abs() + bias.double().abs())
    ref = gelu_ref(x)
    tol = gelu_tol(ref) + 1.13 * dx
    outs = []
    for variant in (1, 3, 4):
        w = f"GELU epilogue {epi} M {M} N {N} K {K} variant {variant}"
        out, _, _ = launch(eng, epi, A, W, variant, bias=bias, what=w, **kw)
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16))
    assert_mutant_far(gelu_ref(x - bias.double()) + bias.double(), ref, tol, ref.numel() // 4, "bias added after GELU")
    eng.close()


@pytest.mark.parametrize("d,N", [(384, 1152), (384, 1536), (1024, 3072), (1024, 4096)])
def test_folded_layernorm_composition(d, N):
    """canonical statistics -> epilogue 5 on W' = bf16(W gamma) against f64 LayerNorm(x) . W'^T + b' (tests/test_gpu_gemm.py (d))"""
    eng = Engine(0)
    eps = 1e-12
    e32 = f32_eps(eps)
    X, fam = ln_rows(d, 99 + d)
    sel = torch.cat([fam["normal"], fam["offset30"], fam["massive"]])
    M = 600
    idx = sel[torch.arange(M, device=DEV) % sel.numel()]
    Xr = X[idx].contiguous()
    g = _gen(1234 + d + N)
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
        w = f"folded LayerNorm d {d} N {N} variant {variant}"
        out, _, _ = launch(eng, 5, Xr, Wp, variant, bias=bp, ln_stats=stats.contiguous(), colsum=colsum, what=w)
        assert_close(out.double(), ref, tol, w)
        outs.append(out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16))
    off = (idx >= 40) & (idx < 80)
    mut = (x * rstd_ref[:, None]) @ Wp.double().T + bp.double()
    assert_mutant_far(mut[off], ref[off], tol[off], int(off.sum()) * N // 2, "colsum ignored")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. two geometries in one process; a second load


def test_two_contexts_alternate_and_reload(crops64):
    solo = {}
    for key in ("S3", "L3"):
        e = _loaded(key)
        e.set_chunk(64)
        solo[key] = [t.clone() for t in _uniform(e, crops64)]
        e.close()
    s, l = _loaded("S3"), _loaded("L3")
    try:
        s.set_chunk(64)
        l.set_chunk(64)
        for turn in range(3):
            for key, e in (("S3", s), ("L3", l), ("L3", l), ("S3", s)):
                e32, e16 = _uniform(e, crops64[: 64 - 7 * turn])
                assert torch.equal(e32, solo[key][0][: 64 - 7 * turn]) and torch.equal(e16, solo[key][1][: 64 - 7 * turn]), (turn, key)
        # a second load replaces the first, whatever the two geometries are: S into the L context, then L back
        assert l.embed_dim == 1024 and len(l.weights_fingerprint()) == 6 + 18 * 3
        l.load_vit(weights_of("S3"))
        assert l.embed_dim == 384 and l.vit_geometry().num_heads == 6
        assert l.weights_fingerprint() == s.weights_fingerprint()
        e32, e16 = _uniform(l, crops64)
        assert torch.equal(e32, solo["S3"][0]) and torch.equal(e16, solo["S3"][1])
        s.load_vit(weights_of("L3"))  # the narrower context regrows its workspace
        e32, e16 = _uniform(s, crops64)
        assert tuple(e32.shape) == (64, 1024) and torch.equal(e32, solo["L3"][0]) and torch.equal(e16, solo["L3"][1])
    finally:
        s.close()
        l.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. downstream


@pytest.mark.parametrize("key", ["L3", "S3"])
def test_downstream_cosine_and_neighbours(key):
    from multimodal_embeddings_amd.cross_compare import cross_compare, to_unit_bf16
    from multimodal_embeddings_amd.region_compare import region_neighbours
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection
    from oracle import compare as oc

    d = GEOMS[key].hidden_size
    eng = _loaded(key)
    try:
        crops = torch.from_numpy(synthetic_crops(256, seed=17)).cuda()
        e32, e16 = _uniform(eng, crops)
        assert tuple(e16.shape) == (256, d)
        rows64 = e16.float().cpu().numpy().astype(np.float64)
        sim = cross_compare(e16, engine=eng)  # bf16 CUDA rows in -> CUDA matrix out
        assert tuple(sim.shape) == (256, 256)
        err = float(np.abs(sim.cpu().numpy().astype(np.float64) - rows64 @ rows64.T).max())
        print(f"cross_compare d {d}: max |gpu - f64| = {err:.3g}")
        assert err <= 2e-6, err
        sim_np = cross_compare(e32.cpu().numpy(), engine=eng)
        assert isinstance(sim_np, np.ndarray) and np.abs(sim_np - oc.cosine_matrix(e32.cpu().numpy())).max() < 1.5e-2
        # region_neighbours over a collection of these rows, 16 pages of 16 regions
        col = RegionCollection()
        ids = [f"region_{r}" for r in range(256)]
        metas = [{"parent_image": f"/data/pages/Paper {r // 16:02d}.png", "region_type": "plain_text", "box_str": "0,0,1,1",
                  "area_percentage": 1.0 + (r % 7), "is_region": True} for r in range(256)]
        col.upsert(ids=ids, embeddings=e32.cpu().numpy().tolist(), metadatas=metas)
        rep = region_neighbours(col, top_n=10, score="cosine", threshold=0.3, engine=eng)
        assert [r["id"] for r in rep] == ids
        unit = to_unit_bf16(e32.cpu().numpy(), eng)  # the rows region_neighbours ranks
        u64 = unit.float().cpu().numpy().astype(np.float64)
        C = eng.cosine(unit, unit).cpu().numpy()
        assert float(np.abs(C.astype(np.float64) - u64 @ u64.T).max()) <= 2e-6
        group = (np.arange(256) // 16).astype(np.int32)
        want_idx, want_sim, _ = oc.neighbour_lists(None, group, top_n=10, fetch=30, sim=C, min_sim=0.3)
        for r, entry in enumerate(rep):
            got = [int(s["id"].split("_")[1]) for s in entry["similar_regions"]]
            assert got == [int(c) for c in want_idx[r] if c >= 0], r
            assert [s["score"] for s in entry["similar_regions"]] == [float(np.float32(v)) for v, c in zip(want_sim[r], want_idx[r]) if c >= 0], r
            assert all(c // 16 != r // 16 for c in got)
        assert sum(len(e["similar_regions"]) for e in rep) >= 256  # the lists are not empty
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusal


def test_unsupported_geometry_is_refused_and_the_context_keeps_its_weights(crops64):
    eng = _loaded("S3")
    try:
        eng.set_chunk(64)
        before32, before16 = [t.clone() for t in _uniform(eng, crops64)]
        fp = eng.weights_fingerprint()
        cases = [
            (ViTGeometry(hidden_size=512, num_layers=1, num_heads=8, intermediate_size=2048), r"\(-1\).*hidden = 512.*384, 768, 1024"),
            (ViTGeometry(hidden_size=1024, num_layers=1, num_heads=8, intermediate_size=4096), r"\(-1\).*heads = 8 at hidden = 1024"),
            (ViTGeometry(hidden_size=384, num_layers=1, num_heads=6, intermediate_size=1000), r"\(-1\).*mlp = 1000"),
        ]
        for geom, pattern in cases:
            w = make_vit_weights(SEED, geom)
            with pytest.raises(MmeError, match=pattern):
                eng.load_vit(w, geom=geom)
            assert eng.embed_dim == 384 and eng.weights_fingerprint() == fp
            e32, e16 = _uniform(eng, crops64)
            assert torch.equal(e32, before32) and torch.equal(e16, before16)
        with pytest.raises(MmeError, match="expected"):  # tensors of another geometry than the one named
            eng.load_vit(weights_of("S3"), geom=L3)
        e32, _ = _uniform(eng, crops64)
        assert torch.equal(e32, before32)
    finally:
        eng.close()
