"""Test infrastructure: whole towers on weights that tell a wrong tower from a right one.

What the two sharpness tests share (tests/test_tower_sharpness_cpu.py, tests/test_gpu_tower_sharpness.py):

  * TOWERS: per case the geometry (two layers), the seed, and the sharp recipe: `make_*_weights(seed, geom, std)` with per-tensor
    factors and offsets applied here, then `round_to_bf16`.  The recipe widens the scores (std 0.05: a 64-wide q.k / 8 of
    order 1 instead of 0.3) and moves the MLP to where the activations differ: fc1.weight x 0.25 and fc1.bias - 2.5 put the
    pre-activations around -2.5 +- 1, fc2.weight x 10 gives what is left of them its weight in the residual back.
  * MUTANTS: per kind of tower, label -> the name the restatements switch on (`mutant=` in tests/*_reference.py).
  * outputs(): every output the GPU test compares, from one pass of the float64 (or emulated) restatement.
  * distance(): per crop or sequence, the maximum over its outputs and their rows of 1 - cos, in float64.
  * TILE_*: the tile tower's case, a registry of its own at the end of this file (tests/test_tile_tower_sharpness_cpu.py,
    tests/test_gpu_tile_tower_sharpness.py), under the same three bounds.

The bounds: an engine within BOUND = 1e-3 of the restatement (the project's bound) is, by the triangle inequality on angles
(1 - cos = 2 sin^2(angle / 2): a factor 4 in 1 - cos is a factor 2 in angle), more than 1e-3 from anything that is MUTANT_FAR
= 4e-3 from the restatement.  EMULATION_NEAR = 2.5e-4 is a condition on the inputs: a restatement that keeps bf16 where the
engine does stays a quarter of the bound from float64, so the bound can be met.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np
import torch

import clip_reference as cr
import clip_text_reference as ctr
import dinov2_reference as dr
import siglip_reference as sr
import siglip_text_reference as strf
import tile_reference as tr
import vit_reference as vr
from multimodal_embeddings_amd import weights as W

BOUND, EMULATION_NEAR, MUTANT_FAR = 1e-3, 2.5e-4, 4e-3
TWO = dict(num_layers=2)
MLP = (("mlp.fc1.weight", 0.25, 0.0), ("mlp.fc1.bias", 1.0, -2.5), ("mlp.fc2.weight", 10.0, 0.0))  # (name suffix, factor, offset)
# Per tower, found on the CPU (what each line is for: the mutants named; measured values in tests/test_tower_sharpness_cpu.py):
# the plain ViT's generator spreads its LayerNorm parameters by std only, so layernorm_before gets a scale of its own
# ("ln1 / ln2 exchanged"), which also widens q and k; at hidden 384 the scores are narrower still ("last / first key dropped")
VIT = MLP + (("layernorm_before.weight", 1.25, 0.0),)
VIT_384 = MLP + (("layernorm_before.weight", 1.5, 0.0), ("q_proj.weight", 1.4, 0.0))
# one key among 197 weighs little: wider queries ("last / first key dropped" at 3e-3 on one crop of three without them)
CLIP = MLP + (("q_proj.weight", 1.5, 0.0),)
# SigLIP adds its positions to a patch embedding with a bias and no LayerNorm behind it: positions of the embedding's own size
# ("position rows rolled by one" 2e-3 and "class row without its position" 4e-4 without it)
SIGLIP = CLIP + (("position_embedding.weight", 8.0, 0.0),)
SIGLIP_TEXT = MLP + (("head.bias", 4.0, 0.0),)  # a head bias of the size of the head's output ("the head's bias left out" 6e-4 without)


@dataclass(frozen=True)
class Tower:
    kind: str  # vit | clip | siglip | dinov2 | clip_text | siglip_text
    geom: object
    seed: int
    std: float = 0.05
    recipe: tuple = MLP
    pos_grid: int | None = None  # DINOv2: the side of the checkpoint's position grid

    @property
    def text(self) -> bool:
        return self.kind.endswith("_text")


MAKE = {"vit": W.make_vit_weights, "clip": W.make_clip_weights, "siglip": W.make_siglip_weights, "dinov2": W.make_dinov2_weights,
        "clip_text": W.make_clip_text_weights, "siglip_text": W.make_siglip_text_weights}
LOADER = {"vit": "load_vit", "clip": "load_clip", "siglip": "load_siglip", "dinov2": "load_dinov2", "clip_text": "load_clip_text",
          "siglip_text": "load_siglip_text"}
VOCAB = 1024  # the text towers: a table small enough to generate in no time; CLIP's EOS is its last id
TOWERS = {
    "vit_b16": Tower("vit", W.ViTGeometry(**TWO), 21, recipe=VIT),
    "vit_b32": Tower("vit", W.ViTGeometry(patch_size=32, **TWO), 22, recipe=VIT),
    "vit_s16": Tower("vit", W.ViTGeometry(hidden_size=384, num_heads=6, intermediate_size=1536, **TWO), 23, recipe=VIT_384),
    "dinov2_b14": Tower("dinov2", W.Dinov2Geometry(**TWO), 24, pos_grid=37),
    "dinov2_1024": Tower("dinov2", W.Dinov2Geometry(hidden_size=1024, num_heads=16, intermediate_size=1024, **TWO), 25),  # ViT-L wide, a narrow MLP
    "clip_b16": Tower("clip", W.CLIPGeometry(**TWO), 26, recipe=CLIP),
    "clip_b32": Tower("clip", W.CLIPGeometry(patch_size=32, **TWO), 27, recipe=CLIP),
    "siglip_b16": Tower("siglip", W.SiglipGeometry(**TWO), 28, recipe=SIGLIP),
    "clip_text": Tower("clip_text", W.CLIPTextGeometry(vocab_size=VOCAB, eos_token_id=VOCAB - 1, **TWO), 29),
    "siglip_text": Tower("siglip_text", W.SiglipTextGeometry(vocab_size=VOCAB, **TWO), 30, recipe=SIGLIP_TEXT),
}

# label (as the issue words it) -> the restatements' switch
ATTENTION = {"uniform attention": "uniform_attention", "Q and K exchanged": "qk_exchanged", "no dh^-0.5": "no_q_scale",
             "heads rolled by one between P and V": "heads_rolled"}
IMAGE = {**ATTENTION, "last key dropped": "last_key_dropped", "first key (class row) dropped": "first_key_dropped",
         "position rows rolled by one": "pos_rolled", "class row without its position": "first_row_without_pos",
         "ln1 / ln2 parameters exchanged": "ln_exchanged", "final LayerNorm left out": "no_final_ln",
         "the neighbouring token pooled": "neighbour_pooled", "residual around the MLP dropped": "no_mlp_residual"}
TEXT = {**ATTENTION, "ln1 / ln2 parameters exchanged": "ln_exchanged", "final LayerNorm left out": "no_final_ln",
        "residual around the MLP dropped": "no_mlp_residual", "position rows rolled by one": "pos_rolled"}
MUTANTS = {
    "vit": IMAGE,
    "clip": {**IMAGE, "pre_layrnorm left out": "no_pre_ln", "erf-GELU for QuickGELU": "other_gelu",
             "projection applied before post_layernorm": "proj_before_post_ln"},
    "dinov2": {**IMAGE, "LayerScale left out": "no_layer_scale", "ls1 / ls2 exchanged": "ls_exchanged",
               "the class position row taken from the interpolated grid": "cls_pos_from_grid"},
    "siglip": {**IMAGE, "probe query unscaled": "probe_unscaled", "the head's MLP residual dropped": "no_head_mlp_residual",
               "post_layernorm left out of the K | V input": "kv_without_post_ln", "mean pooling for the head": "mean_pooled_head"},
    "clip_text": {**TEXT, "causal mask dropped": "no_causal_mask", "pooled at the last position for the EOS position": "pooled_last",
                  "pooled one before EOS": "pooled_before_eos", "erf-GELU for QuickGELU": "other_gelu"},
    "siglip_text": {**TEXT, "padding masked out": "padding_masked", "position 62 pooled for 63": "pooled_62",
                    "the head's bias left out": "no_head_bias"},
}
PATCH32 = {"patch columns in (ky, kx, c) order": "patch_kykxc"}
# the one mutant that is recorded and not asserted: tanh-GELU against erf-GELU, in the towers that run one of the two.  The
# kernel-level tests that hold the two forms apart element by element: tests/test_gpu_gemm.py (erf-GELU epilogues, mutant
# "tanh-GELU") and tests/test_gpu_siglip.py (tanh-GELU epilogues, mutant "erf-GELU").
RECORDED_ONLY = {"tanh-GELU against erf-GELU": "other_gelu"}


def mutants_of(key: str) -> dict:
    t = TOWERS[key]
    return {**MUTANTS[t.kind], **(PATCH32 if getattr(t.geom, "patch_size", 16) == 32 else {})}


def recorded_only_of(key: str) -> dict:
    return {} if TOWERS[key].kind.startswith("clip") else RECORDED_ONLY


def weights_of(key: str, sharp: bool = True) -> dict:
    """The sharp weights of a case; sharp=False: the same seed at std 0.02 without the recipe, what the other tests use"""
    t = TOWERS[key]
    kw = {"pos_grid": t.pos_grid} if t.pos_grid else {}
    w = MAKE[t.kind](t.seed, t.geom, std=t.std if sharp else 0.02, **kw)
    if sharp:
        for name in w:
            for suffix, factor, offset in t.recipe:
                if name.endswith(suffix):
                    w[name] = W.round_to_bf16(w[name] * np.float32(factor) + np.float32(offset)).reshape(w[name].shape)
    return w


def geom_of(key: str):
    t = TOWERS[key]
    return dataclasses.replace(t.geom, position_grid=t.pos_grid) if t.pos_grid else t.geom


N_CROPS, N_SEQ = 3, 8


def inputs_of(key: str):
    """Image towers: (uint8 crops [3, 224, 224, 3], pixel values f32 [3, 3, 224, 224]).  Text towers: ids [8, T] of eight
    different lengths, the shortest and the longest the tower takes among them."""
    from oracle import preprocess as opre

    t = TOWERS[key]
    if t.kind == "clip_text":
        return W.synthetic_token_ids(N_SEQ, VOCAB, VOCAB - 1, seed=t.seed, lengths=[1, 2, 9, 31, 32, 33, 76, 77])
    if t.kind == "siglip_text":
        return W.siglip_token_ids(N_SEQ, VOCAB, t.geom.pad_token_id, seed=t.seed, lengths=[1, 2, 9, 31, 33, 62, 63, 64])
    crops = W.synthetic_crops(N_CROPS, seed=t.seed)
    return crops, np.stack([opre.preprocess_crop(a) for a in crops]).astype(np.float32)


def _rows(x) -> np.ndarray:
    """[n, D] or [n, T, D] -> float64 [n, T, D]"""
    x = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    return x[:, None, :] if x.ndim == 2 else x


@torch.no_grad()
def outputs(key: str, w: dict, x, dtype=torch.float64, mutant=None) -> dict:
    """name -> float64 [n, rows, D] of every output the GPU test compares, from one pass through the restatement.
    Image towers: "tokens" (every row behind the final LayerNorm), "pooled 0" and "pooled last" (the engine's embedding under
    the two pool tokens: image_embeds for CLIP with a projection); SigLIP: "tokens" and "head".  Text towers: "text".
    `x`: the pixel values or the ids of `inputs_of`."""
    t, geom = TOWERS[key], geom_of(key)
    if t.kind == "clip_text":
        pooled, proj = ctr.clip_text_forward(x, w, geom, dtype, mutant=mutant)
        return {"text": _rows(proj if proj is not None else pooled)}
    if t.kind == "siglip_text":
        return {"text": _rows(strf.siglip_text_forward(x, w, geom, dtype, mutant=mutant))}
    last = geom.seq_len - 1
    if t.kind == "siglip":
        hs = sr.siglip_hidden_states(x, w, geom, dtype, mutant)
        return {"tokens": _rows(cr.final_rows(hs, *sr._post_ln(w, dtype), geom.layer_norm_eps, mutant)),
                "head": _rows(sr.siglip_head(hs, w, geom, dtype, mutant))}
    if t.kind == "clip":
        hs = cr.clip_hidden_states(x, w, geom, dtype, mutant)
        out = {"tokens": _rows(cr.final_rows(hs, *cr._post_ln(w, dtype), geom.layer_norm_eps, mutant))}
        for name, tok in (("pooled 0", 0), ("pooled last", last)):
            po, proj = cr.clip_pool(hs, w, geom, dtype, tok, mutant)
            out[name] = _rows(proj if proj is not None else po)
        return out
    mod, hidden, pool = (dr, dr.dinov2_hidden_states, dr.dinov2_pool) if t.kind == "dinov2" else (vr, vr.vit_hidden_states, vr.vit_pool)
    hs = hidden(x, w, geom, dtype, mutant=mutant)
    out = {"tokens": _rows(cr.final_rows(hs, *mod._final_ln(w, dtype), geom.layer_norm_eps, mutant))}
    for name, tok in (("pooled 0", 0), ("pooled last", last)):
        out[name] = _rows(pool(hs, w, geom, dtype, tok, mutant))
    return out


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float64 [n, rows, D] x 2 -> 1 - cos per row [n, rows]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def distance(got: dict, want: dict) -> np.ndarray:
    """The metric: per crop or sequence, the maximum of 1 - cos over every row of every output, [n] in float64"""
    assert got.keys() == want.keys()
    return np.max([one_minus_cos(got[k], want[k]).max(axis=1) for k in want], axis=0)


# ---- the tile tower (tests/test_tile_tower_sharpness_cpu.py, tests/test_gpu_tile_tower_sharpness.py) -------------------------
# A registry of its own beside TOWERS and MUTANTS: one image is one sequence of 6432 tokens with an aspect-ratio id and a tile
# count, and a forward of the restatement (tests/tile_reference.py) takes seconds, so the cases are three images, not ten towers.
# The smallest tower with a local layer, a gated global layer and an intermediate feature (token counts and widths are fixed
# at compile time in the engine: nothing smaller exists)
TILE_GEOM = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
TILE_SEED = 31
# (name suffix, factor, offset); a gate is SET by factor 0.  What each line is for (the mutants named; measured values in
# tests/test_tile_tower_sharpness_cpu.py).  The seeded gates are pi / 4 twice: "gate_attn / gate_ffn exchanged" is the same tower.
TILE_RECIPE = MLP + (
    # scores x 16 (the weights are N(0, 0.02) at width 1280), the factor of the peaked-attention test of tests/test_gpu_tilevit.py.
    # At x 2.5 (scores x 6.25) "one key of 6432 dropped" is 2.8e-3 and "a tile's 7 padding tokens taken as real" 1.3e-3, at
    # x 3.5 7.0e-3 and 3.7e-3; at x 5 the bf16 emulation leaves its bound (2.9e-4)
    ("q_proj.weight", 4.0, 0.0), ("k_proj.weight", 4.0, 0.0),
    # two different gates, one of them where g and tanh g are apart (1.5 against 0.905): "exchanged", "without its tanh"
    ("gate_attn", 0.0, 1.5), ("gate_ffn", 0.0, 0.3),
    # the post-tile embedding at the size of the LayerNorm output it is added to (N(0, 0.02) x tanh(-0.5) is 1 % of it): "left
    # out" 6e-5 and "added before layernorm_post" 2e-6 without it
    ("post_tile_positional_embedding.embedding.weight", 50.0, 0.0),
    # layernorm_post with a spread: gamma 1 + N(0, 0.5), beta N(0, 0.5).  The global layer normalises its input again, so a
    # layernorm_post of gamma near 1 and beta near 0 is nearly invisible: "layernorm_post left out" 9e-4 without it
    ("layernorm_post.weight", 25.0, -24.0), ("layernorm_post.bias", 25.0, 0.0),
    # ln1 apart from ln2, gamma 1 + N(0, 0.2): "ln1 / ln2 parameters exchanged" 1.1e-3 without it
    ("input_layernorm.weight", 10.0, -9.0),
)
TILE_IMAGES = ((300, 200, 3), (400, 900, 3), (1000, 1100, 3))  # 1, 2 and 4 tiles; aspect-ratio ids 1, 2 and 6
TILE_MUTANTS = {
    **ATTENTION,
    "padding keys masked for every query": "pad_keys_masked", "(padding, padding) mask dropped": "no_pad_mask",
    "each tile attends only itself": "tile_local", "global gates ignored": "gates_ignored",
    "gate used without its tanh": "gate_without_tanh", "gate_attn / gate_ffn exchanged": "gates_exchanged",
    "pre-tile embedding added to the class row too": "pre_on_class", "(1 - tanh g) factor dropped": "no_one_minus_gate",
    "tile-embedding rows rolled by one tile": "tile_emb_rolled", "post-tile embedding left out": "no_post_emb",
    "post-tile embedding added before layernorm_post": "post_emb_before_ln", "layernorm_pre left out": "no_ln_pre",
    "layernorm_post left out": "no_ln_post", "ln1 / ln2 parameters exchanged": "ln_exchanged",
    "residual around the MLP dropped": "no_mlp_residual", "the class row of tile 1 pooled for tile 0": "pooled_tile_1",
    "a tile's 7 padding tokens taken as real": "pad_tokens_real", "one key of 6432 dropped": "key_dropped",
}
# recorded and not asserted (tests/test_tile_tower_sharpness_cpu.py says which levers were tried and what holds the property)
TILE_RECORDED_ONLY = {"tanh-GELU for erf-GELU": "other_gelu"}


def tile_weights(sharp: bool = True, recipe=TILE_RECIPE) -> dict:
    """The sharp weights of the tile case; sharp=False: `make_tile_vit_weights` of the same seed as the tile tests use them"""
    w = dict(W.make_tile_vit_weights(TILE_SEED, TILE_GEOM))
    if sharp:
        for name in w:
            for suffix, factor, offset in recipe:
                if name.endswith(suffix):
                    w[name] = W.round_to_bf16(w[name] * np.float32(factor) + np.float32(offset)).reshape(w[name].shape)
        assert all(float(v[0]) != 0.0 for name, v in w.items() if name.endswith("gate") or ".gate_" in name)
    return w


def tile_images() -> list:
    """Three synthetic uint8 images that the Mllama preprocessing turns into 1, 2 and 4 tiles"""
    rng = np.random.default_rng(TILE_SEED)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in TILE_IMAGES]


def tile_inputs() -> list:
    """Per image (pixel values f32 [4, 3, 560, 560], aspect-ratio id, tile count) from the oracle's tile preprocessing, which
    `mme_preprocess_tiles` equals bit for bit (tests/test_gpu_tiles.py)"""
    from oracle import preprocess as opre

    return [opre.preprocess_tiles(a)[:3] for a in tile_images()]


def tile_distance(got: dict, want: dict) -> float:
    """The metric of one image: the maximum of 1 - cos over every row of all four tiles of every output, in float64"""
    assert got.keys() == want.keys()
    return float(max(one_minus_cos(got[k], want[k]).max() for k in want))
