"""Token rows out of the forward (mme_vit_tokens / mme_embed_tokens) on the GPU.

One-layer seeded towers at hidden 384 (MLP 64, as TINY of tests/test_gpu_dinov2.py), five crops through chunks of two:
(a) token row t = the bf16 output of mme_vit_forward(pool_token = tok0 + t), bit for bit, at the first row, 31, 32, 33 and the
    last, with forward pruning on and off (ViT/16, ViT/32, DINOv2, CLIP without projection);
(b) the pooled outputs of the token call = mme_vit_forward's, bit for bit (CLIP with projection and SigLIP included), and the
    pruning setting is what it was afterwards: a plain forward still launches the pruned sequence;
(c) mme_embed_tokens = mme_preprocess + mme_vit_tokens, bit for bit; a one-row window at the last token; sentinel items stay;
(d) every token row against transformers' last_hidden_state (tests/golden/tokens_<tower>.npz, CLIP behind its post_layernorm),
    L2-normalised in float64: max(1 - cos) <= 1e-3, the project's bound for the bf16 path (what that bound cannot see on
    std 0.02 weights -- uniform attention, Q and K exchanged, a dropped key -- is held by tests/test_gpu_tower_sharpness.py);
(e) the refusals, by message;
(f) RegionEmbedder.get_patch_embeddings: the vectors of get_image_embeddings, the token blocks of mme_embed_tokens in input
    order, zeros for an item that failed, the caller's `out`.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_tokens_golden as mkt  # noqa: E402
from test_gpu_gemm import BF16, DEV, Guard, assert_bits  # noqa: E402

from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIPGeometry, Dinov2Geometry, SiglipGeometry, ViTGeometry, make_clip_weights,  # noqa: E402
                                               make_dinov2_weights, make_siglip_weights, make_vit_weights, synthetic_crops)

pytestmark = pytest.mark.gpu

I16 = torch.int16
SMALL = dict(hidden_size=384, num_layers=1, num_heads=6, intermediate_size=64)
# tower -> (loader, geometry, weight generator, tokens, index of the first patch token)
TOWERS = {
    "vit16": ("load_vit", ViTGeometry(**SMALL), make_vit_weights, 197, 1),
    "vit32": ("load_vit", ViTGeometry(patch_size=32, **SMALL), make_vit_weights, 50, 1),
    "dinov2": ("load_dinov2", Dinov2Geometry(**SMALL), make_dinov2_weights, 257, 1),
    "clip": ("load_clip", CLIPGeometry(**SMALL, projection_dim=None), make_clip_weights, 197, 1),
    "clip_proj": ("load_clip", CLIPGeometry(**SMALL, projection_dim=256), make_clip_weights, 197, 1),
    "siglip": ("load_siglip", SiglipGeometry(**SMALL), make_siglip_weights, 196, 0),
}
N, D = 5, 384
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
def crops():
    """(pix, offs, hw) of five crops: three of 224 x 224, two ragged"""
    rng = np.random.default_rng(3)
    arrays = list(synthetic_crops(3, seed=5)) + [rng.integers(0, 256, s, dtype=np.uint8) for s in [(90, 300, 3), (333, 120, 3)]]
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(N, dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(DEV), offs, hw


def tower(key, seed=7):
    loader, geom, make, T, first = TOWERS[key]
    eng = Engine(0)
    getattr(eng, loader)(make(seed, geom), geom=geom)
    eng.set_chunk(2)  # five crops: three chunks, the last of one crop
    return eng, T, first


def bits(t):
    return t.contiguous().view(I16)


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("key", ["vit16", "vit32", "dinov2", "clip"])
def test_token_rows_are_the_pooled_rows_of_the_forward(crops, key, prune):
    eng, T, first = tower(key)
    try:
        eng.set_forward_pruning(prune)
        patches = eng.preprocess(*crops)
        tokens, _, _ = eng.vit_tokens(patches, tok0=0, ntok=T)
        assert tuple(tokens.shape) == (N, T, D) and tokens.dtype == BF16
        for t in (0, 31, 32, 33, T - 1):
            _, e16 = eng.vit_forward(patches, pool_token=t, want_f32=False)
            torch.cuda.synchronize()
            assert_bits(bits(tokens[:, t]), bits(e16), f"{key} prune {prune}: token row {t} against mme_vit_forward(pool_token = {t})")
        assert not torch.equal(bits(tokens[:, 31]), bits(tokens[:, 32])), "neighbouring rows differ: an off-by-one row would show"
        # the default window is the patch tokens; any window is that slice of the rows
        patch_rows, _, _ = eng.vit_tokens(patches)
        assert tuple(patch_rows.shape) == (N, T - first, D)
        assert_bits(bits(patch_rows), bits(tokens[:, first:]), f"{key}: the default window")
        win, _, _ = eng.vit_tokens(patches, tok0=31, ntok=3)
        assert_bits(bits(win), bits(tokens[:, 31:34]), f"{key}: the window 31..33")
    finally:
        eng.close()


@pytest.mark.parametrize("key", list(TOWERS))
def test_pooled_outputs_equal_the_forward_and_pruning_stays_set(crops, key):
    eng, T, first = tower(key)
    try:
        patches = eng.preprocess(*crops)
        for prune in (False, True):
            eng.set_forward_pruning(prune)
            for pool in (0, T - 1):
                w32, w16 = eng.vit_forward(patches, pool_token=pool)
                _, e32, e16 = eng.vit_tokens(patches, pool_token=pool)
                torch.cuda.synchronize()
                assert tuple(e32.shape) == (N, eng.embed_dim)
                assert_bits(e32.view(torch.int32), w32.view(torch.int32), f"{key} prune {prune} pool {pool}: emb_f32")
                assert_bits(bits(e16), bits(w16), f"{key} prune {prune} pool {pool}: emb_bf16")
        # the setting reads back through what a plain forward launches: the pruned last layer gathers and scatters the pooled
        # rows (pooling-class launches a full pass does not make); a token pass in between changes nothing
        if key != "siglip":  # (SigLIP's head reads every row: the setting has no effect there)
            counts = {}
            for name, prune, token_pass in (("full", False, False), ("pruned", True, False), ("pruned, after a token pass", True, True)):
                eng.set_forward_pruning(prune)
                if token_pass:
                    eng.vit_tokens(patches)
                eng.profile(True)
                eng.vit_forward(patches)
                counts[name] = {k: v[1] for k, v in eng.profile_read().items()}
                eng.profile(False)
            assert counts["pruned"] != counts["full"] and counts["pruned, after a token pass"] == counts["pruned"], counts
    finally:
        eng.close()


@pytest.mark.parametrize("key", ["vit16", "vit32", "dinov2", "siglip"])
def test_embed_tokens_is_preprocess_then_vit_tokens(crops, key):
    eng, T, first = tower(key)
    try:
        patches = eng.preprocess(*crops)
        want, w32, w16 = eng.vit_tokens(patches, pool_token=T - 1)
        ntok = T - first
        out = Guard(BF16, N * ntok, D, guard=ntok)  # one whole item of sentinel rows on either side
        got, e32, e16 = eng.embed_tokens(*crops, pool_token=T - 1, out=out.view.view(N, ntok, D))
        torch.cuda.synchronize()
        out.check(f"{key}: the items before and after")
        assert_bits(out.valid_bits(), bits(want).view(N * ntok, D), f"{key}: embed_tokens against preprocess + vit_tokens")
        assert_bits(e32.view(torch.int32), w32.view(torch.int32), f"{key}: emb_f32")
        assert_bits(bits(e16), bits(w16), f"{key}: emb_bf16")
        one = Guard(BF16, N, D, guard=1)
        eng.embed_tokens(*crops, tok0=T - 1, ntok=1, out=one.view.view(N, 1, D), want_f32=False, want_bf16=False)
        torch.cuda.synchronize()
        one.check(f"{key}: a one-row window")
        assert_bits(one.valid_bits(), bits(want[:, -1]), f"{key}: the window of the last token alone")
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(mkt.CASES))
def test_token_rows_against_transformers_last_hidden_state(name):
    """Two seeded crops through two-layer towers at hidden 384: every row of the recorded last_hidden_state, L2-normalised in
    float64, against the engine's row."""
    import make_clip_golden as mkc

    geom, w = mkt.weights_of(name)
    rec = np.load(mkt.out_path(name))["tokens"].astype(np.float64)
    T = rec.shape[1]
    rec /= np.linalg.norm(rec, axis=2, keepdims=True)
    arrays = synthetic_crops(mkc.N_CROPS, seed=mkc.CROP_SEED)[: mkt.N_CROPS]
    eng = Engine(0)
    try:
        getattr(eng, {"vit": "load_vit", "dinov2": "load_dinov2", "siglip": "load_siglip", "clip": "load_clip"}[name])(w, geom=geom)
        per = 224 * 224 * 3
        pix = torch.from_numpy(np.ascontiguousarray(arrays)).to(DEV).reshape(-1)
        offs, hw = np.arange(mkt.N_CROPS, dtype=np.int64) * per, np.full((mkt.N_CROPS, 2), 224, dtype=np.int32)
        tokens, _, _ = eng.embed_tokens(torch.cat([pix, pix.new_zeros(16)]), offs, hw, tok0=0, ntok=T)
        torch.cuda.synchronize()
    finally:
        eng.close()
    got = tokens.double().cpu().numpy()
    assert got.shape == rec.shape
    assert np.abs(np.linalg.norm(got, axis=2) - 1.0).max() <= 2.0**-7, "unit rows up to the bf16 rounding"
    err = 1.0 - np.sum(got * rec, axis=2) / np.linalg.norm(got, axis=2)
    print(f"{name}: max(1 - cos) over {err.size} token rows = {err.max():.3g}")
    assert err.max() <= 1e-3, (name, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    # the rows are told apart: against the row before, the recorded rows are far
    shifted = 1.0 - np.sum(got[:, 1:] * rec[:, :-1], axis=2)
    assert np.median(shifted) > 0.05


def test_refusals_name_the_argument(crops):
    bare = Engine(0)
    try:
        dummy = torch.zeros((2 * 196, 768), dtype=BF16, device=DEV)
        with pytest.raises(MmeError, match="mme_vit_tokens: call mme_load_vit first"):
            bare.vit_tokens(dummy)
        with pytest.raises(MmeError, match="mme_embed_tokens: call mme_load_vit first"):
            bare.embed_tokens(*crops)
    finally:
        bare.close()
    eng, T, _ = tower("vit16")
    try:
        patches = eng.preprocess(*crops)
        for kw, text in [(dict(tok0=-1, ntok=3), "tok0 -1, ntok 3; supported tok0 >= 0, ntok >= 1, tok0 \\+ ntok <= 197"),
                         (dict(tok0=0, ntok=0), "tok0 0, ntok 0"), (dict(tok0=190, ntok=8), "tok0 190, ntok 8"),
                         (dict(pool_token=197), "pool_token 197 outside 0..196")]:
            with pytest.raises(MmeError, match="mme_vit_tokens: .*" + text):
                eng.vit_tokens(patches, **kw)
            with pytest.raises(MmeError, match="mme_embed_tokens: .*" + text):
                eng.embed_tokens(*crops, **kw)
        rc = eng.lib.mme_vit_tokens(eng.h, patches.data_ptr(), N, 0, 1, 196, None, None, None, None)
        assert rc != 0 and b"tokens_bf16_dev is NULL" in eng.lib.mme_last_error(eng.h)
    finally:
        eng.close()


def test_a_tile_vit_context_is_refused():
    from multimodal_embeddings_amd.weights import TILE_VIT, make_tile_vit_weights

    geom = dataclasses.replace(TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
    eng = Engine(0)
    try:
        eng.load_tile_vit(make_tile_vit_weights(5, geom), geom)
        out = torch.zeros((1, 196, 768), dtype=BF16, device=DEV)
        rc = eng.lib.mme_vit_tokens(eng.h, out.data_ptr(), 1, 0, 1, 196, out.data_ptr(), None, None, None)
        assert rc != 0 and b"mme_vit_tokens: encoder tile_vit; supported: the single-tile image towers" in eng.lib.mme_last_error(eng.h)
    finally:
        eng.close()


def test_get_patch_embeddings_returns_vectors_and_token_blocks(crops, tmp_path):
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    _, geom, make, T, first = TOWERS["dinov2"]
    rng = np.random.default_rng(9)
    good = list(synthetic_crops(9, seed=2)) + [rng.integers(0, 256, s, dtype=np.uint8) for s in [(60, 400, 3), (500, 77, 3)]]
    items = good[:4] + [str(tmp_path / "missing.png")] + good[4:]  # item 4 cannot be read: a None hole, a block of zeros
    emb = RegionEmbedder(device=0, encoder="dinov2", weights=make(7, geom), geometry=geom, chunk=4)
    try:
        vectors, tokens = emb.get_patch_embeddings(items)
        assert vectors == emb.get_image_embeddings(items) and vectors[4] is None and sum(v is None for v in vectors) == 1
        assert tuple(tokens.shape) == (len(items), T - first, D) and tokens.dtype == BF16 and tokens.is_cuda
        assert not bool(tokens[4].view(I16).any()), "a failed item's block is zeros"
        pix, offs, hw = emb.pack(good)
        want, _, _ = emb.engine.embed_tokens(pix, offs, hw, emb.pool_token)
        torch.cuda.synchronize()
        keep = [i for i in range(len(items)) if i != 4]
        assert_bits(bits(tokens[keep]).view(len(good), -1), bits(want).view(len(good), -1), "token blocks in input order")
        out = torch.full((len(items), T - first, D), 3.0, dtype=BF16, device=DEV)
        v2, t2 = emb.get_patch_embeddings(items, out=out)
        assert t2 is out and v2 == vectors and torch.equal(out.view(I16), tokens.view(I16))
        with pytest.raises(ValueError, match="`out` must be a contiguous bfloat16 CUDA tensor"):
            emb.get_patch_embeddings(items, out=out[:, :5])
    finally:
        for e in emb.engines:
            e.close()
