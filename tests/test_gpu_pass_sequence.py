"""The launch sequence of one encoder pass, pinned by the profiler's scope counts (csrc/encoder_pass.hip writes the
transformer block once; the three towers set its parameters).  With profiling on, every launch of the pass sits in one
scope of its class, so `Engine.profile_read()` after one forward of one chunk counts the launches per class.  The closed
forms below are read off the sequence, NL layers deep:

  image tower      gemm: patch embedding + 4 per block (+ the projection); layernorm: the [CLS] rows (the token rows at
                   patch 32), the first statistics pass (CLIP: pre_layrnorm), two per block less the one no block follows;
                   pool: one launch, CLIP with projection pool-LN + L2, a pruned last layer two more (gather, scatter)
  text tower       preprocess: the token rows; gemm: 4 per block (+ the projection); layernorm: the first statistics pass
                   and two per block less the last; pool: EOS pool-LN + L2
  tile tower       L local + G global blocks, T = L + G: preprocess: patchify; gemm: patch embedding + 4 T; layernorm:
                   assembly, the first statistics pass, 2 T less the one after the last block, and where G > 0
                   layernorm_post, whose statistics pass replaces the one after the last local block: one more in all

The cases run ln_mode 0 or 1: no partial planes, so no count depends on which GEMM kernel the launcher picks.  Under
ln_mode 2 only the gemm and attention counts are held to mode 1's, and the embeddings to mode 1's bits.
"""
import dataclasses

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import weights as W
from multimodal_embeddings_amd._lib import Engine

pytestmark = pytest.mark.gpu

NL = 2
CLASSES = ("preprocess", "gemm", "layernorm", "attention", "pool")


def counted(e, forward):
    """({class: scopes} of one call of `forward` with profiling on, what it returned)"""
    e.profile(True)
    out = forward()
    counts = {k: int(v[1]) for k, v in e.profile_read().items()}
    e.profile(False)
    assert all(counts[k] == 0 for k in counts if k not in CLASSES), counts
    return {k: counts[k] for k in CLASSES}, out


def patches_of(e, n):
    crops = W.synthetic_crops(n, seed=5)
    offs = np.arange(n, dtype=np.int64) * crops[0].size  # 150 528 bytes per crop: every crop 16-byte aligned
    hw = np.full((n, 2), 224, dtype=np.int32)
    return e.preprocess(torch.from_numpy(crops.reshape(-1)).to("cuda:0"), offs, hw)


IMAGE_TOWERS = {
    "vit_b16": (W.VIT_B16, Engine.load_vit, W.make_vit_weights), "vit_b32": (W.VIT_B32, Engine.load_vit, W.make_vit_weights),
    "clip_b16": (W.CLIP_B16, Engine.load_clip, W.make_clip_weights), "siglip_b16": (W.SIGLIP_B16, Engine.load_siglip, W.make_siglip_weights),
    "dinov2_b14": (W.DINOV2_B14, Engine.load_dinov2, W.make_dinov2_weights),
}


@pytest.mark.parametrize("name", list(IMAGE_TOWERS))
def test_image_pass(name):
    """3 crops at patch 16 are 591 rows (588 without a class token), 6 at patch 32 are 300: two 256-row panels and a ragged
    tail; 3 at patch 14 are 771: three panels and a ragged 3.  One chunk.

    SigLIP, modes 0 and 1: gemm = patch embedding + 4 per block + the head's K | V, out_proj, fc1, fc2; layernorm = the
    token rows + two per block + two for the head (mode 0: its two LayerNorm launches; mode 1: the first statistics pass
    and the one behind out_proj, every block being followed by a folded LayerNorm); pool = map_pool with the zeroed
    residual, then L2.  DINOv2: vit_b16's closed form (the token rows in place of the [CLS] rows).  Both closed forms
    were read off the sequence and then confirmed by the counts of the library before the image pass was split into
    stem, blocks and tail."""
    base, load, make = IMAGE_TOWERS[name]
    geom = dataclasses.replace(base, num_layers=NL)
    clip, sig = name == "clip_b16", name == "siglip_b16"
    e = Engine(0)
    try:
        load(e, make(11, geom), geom=geom)
        patches = patches_of(e, 6 if geom.patch_size == 32 else 3)
        want = {"preprocess": 0, "gemm": 1 + 4 * NL + (1 if clip else 0), "layernorm": 2 * NL + 1, "attention": NL, "pool": 2 if clip else 1}
        if sig:
            want = {"preprocess": 0, "gemm": 4 * NL + 5, "layernorm": 2 * NL + 3, "attention": NL, "pool": 2}
        got = {}
        for mode in (1, 2) if clip else (0, 1, 2):
            e.set_ln_fusion(mode)
            got[mode] = counted(e, lambda: e.vit_forward(patches))
        assert got[1][0] == want
        if not clip:
            assert got[0][0] == want
        assert all(got[2][0][k] == got[1][0][k] for k in ("gemm", "attention")), got[2][0]
        assert torch.equal(got[2][1][0], got[1][1][0]) and torch.equal(got[2][1][1], got[1][1][1])
        if name == "vit_b16":  # the pruned last layer: the same block on the gathered rows, between a gather and a scatter
            e.set_ln_fusion(1)
            e.set_forward_pruning(True)
            pruned, out = counted(e, lambda: e.vit_forward(patches))
            assert pruned == dict(want, pool=3)
            assert torch.equal(out[0], got[1][1][0])
            # a token pass with pruning on runs the last block unpruned: no gather, no scatter, one more pool scope (the token rows)
            tokens, out = counted(e, lambda: e.vit_tokens(patches))
            assert tokens == dict(want, pool=2)
            assert torch.equal(out[1], got[1][1][0]) and torch.equal(out[2], got[1][1][1])
    finally:
        e.close()


@pytest.mark.parametrize("proj", [512, None])
def test_text_pass(proj):
    geom = W.CLIPTextGeometry(num_layers=NL, vocab_size=256, eos_token_id=255, projection_dim=proj)
    e = Engine(0)
    try:
        e.load_clip_text(W.make_clip_text_weights(41, geom), geom)
        ids = W.synthetic_token_ids(3, geom.vocab_size, geom.eos_token_id, 7)
        got, _ = counted(e, lambda: e.text_forward(ids))
        assert got == {"preprocess": 1, "gemm": 4 * NL + (1 if proj else 0), "layernorm": 2 * NL, "attention": NL, "pool": 2}
    finally:
        e.close()


@pytest.mark.parametrize("local, glob", [(1, 1), (2, 0)])
def test_tile_pass(local, glob):
    geom = dataclasses.replace(W.TILE_VIT, num_layers=local, num_global_layers=glob, intermediate_layers=(0,))
    T = local + glob
    e = Engine(0)
    try:
        e.load_tile_vit(W.make_tile_vit_weights(3, geom), geom)
        pv = torch.from_numpy(W.irwin_hall_normal(9, 0, 4 * 3 * 560 * 560).reshape(1, 4, 3, 560, 560)).to("cuda:0")
        got = {}
        for mode in (1, 2):
            e.set_ln_fusion(mode)
            got[mode] = counted(e, lambda: e.tile_vit_forward(pv, [6], [4]))  # aspect-ratio id 6: 2 x 2 tiles
        assert got[1][0] == {"preprocess": 1, "gemm": 1 + 4 * T, "layernorm": 2 * T + 1 + (1 if glob else 0), "attention": T, "pool": 1}
        assert all(got[2][0][k] == got[1][0][k] for k in ("gemm", "attention")), got[2][0]
        assert torch.equal(got[2][1][1], got[1][1][1]) and torch.equal(got[2][1][2], got[1][1][2])
    finally:
        e.close()
