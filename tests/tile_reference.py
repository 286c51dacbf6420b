"""Test infrastructure: the tile tower (oracle/mllama_vision.py) with a choice of `dtype` and the mutant switches of
tests/tower_mutants.py (TILE_MUTANTS), as tests/vit_reference.py is to oracle/vit.py.  oracle/mllama_vision.py stays what
tests/test_oracle_pins.py pins to transformers; tests/test_tile_tower_sharpness_cpu.py holds this file to it bit for bit in
float32 with `mutant=None` (the operations and their order are the oracle's, the attention one head at a time included).

`mutant="bf16"` is no wrong tower but the emulation: float32 arithmetic, values rounded to bf16 (nearest even) wherever the
engine stores bf16.  What each `stored(...)` below stands for:

    the patch matrix                       csrc/tilevit.hip tile_patchify          `dst[e] = (bf16_t)v`
    the patch embedding                    csrc/capi_tilevit.hip mme_tile_vit_forward   the EPI_BIAS GEMM into `t->pemb` (bf16)
    x behind assembly and layernorm_pre    csrc/tilevit.hip tile_assemble          `o[k] = (bf16_t)((v[j + k] - st.mean) * st.rstd * gv[k] + bv[k])`
                                           (the sums before the LayerNorm stay in f32 registers)
    q | k | v                              csrc/encoder_pass.hip EncoderPass::qkv_ln    `g.out = qkv` (EPI_LN_BIAS, bf16 rows)
    the attention output                   csrc/capi_tilevit.hip                   launch_attention_tiles(t->qkv.p, t->att.p, ...)
    x behind the attention residual add    csrc/encoder_pass.hip EncoderPass::residual  `g.out = xr; g.res = xr` (from after_attention, o_w)
    the activation output                  csrc/encoder_pass.hip EncoderPass::fc1_ln    `g.out = mlp` (EPI_LN_BIAS_GELU)
    x behind the MLP residual add          csrc/encoder_pass.hip EncoderPass::residual  the same epilogue with fc2_w; the saved intermediate
                                           states and the final state are copies of this x
    x behind layernorm_post + post-tile    csrc/tilevit.hip tile_ln_post           `o[k] = (bf16_t)(... * gv[k] + bv[k] + po[k])`

Not emulated: the roundings of the prepared WEIGHTS (LayerNorm gamma and the tanh gates folded into a matrix before it is
rounded to bf16, csrc/capi_tilevit.hip prepare_tile), and q rounded with dh^-0.5 log2(e) already in it.

The wrong towers (`mutant=` one name or a collection; the labels are in tests/tower_mutants.py):

    attention   uniform_attention, qk_exchanged, no_q_scale, heads_rolled, pad_keys_masked (padding keys masked for every query),
                no_pad_mask ((padding, padding) mask dropped), tile_local (a query sees the keys of its own tile only),
                pad_tokens_real (only the padding TILES count as padding), key_dropped (key 1, the first patch of tile 0)
    blocks      ln_exchanged, no_mlp_residual, other_gelu (tanh-GELU)
    stem        pre_on_class, no_one_minus_gate, tile_emb_rolled, no_ln_pre
    tail        no_post_emb, post_emb_before_ln, no_ln_post                                          } LOCAL_FREE: the stem and the
    global      gates_ignored, gate_without_tanh (the two gates of a global layer), gates_exchanged   } local stack are the
    pooling     pooled_tile_1                                                                         } restatement's own
"""
from __future__ import annotations

import math

import numpy as np
import torch

from clip_reference import has, stored
from multimodal_embeddings_amd.weights import TILE_VIT, TileViTGeometry
from oracle.mllama_vision import padding_flags

# mutants that leave the stem and the local layers alone: `local_state` of the restatement itself may be handed to them
LOCAL_FREE = frozenset({"no_post_emb", "post_emb_before_ln", "no_ln_post", "gates_ignored", "gate_without_tanh", "gates_exchanged",
                        "pooled_tile_1"})
DROPPED_KEY = 1


def _t(w, name, dtype):
    return torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dtype)


def _ln(x, g, b, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, eps)


def _tanh_gate(w, name) -> float:
    return math.tanh(float(w[name][0]))


def masked_pairs(num_tiles: int, geom: TileViTGeometry = TILE_VIT, mutant=None):
    """bool [T, T] (query, key): the pairs that get finfo(float32).min, or None when nothing is masked"""
    pad = padding_flags(num_tiles, geom)
    if has(mutant, "pad_tokens_real"):
        pad = (torch.arange(geom.max_num_tiles)[:, None] >= num_tiles).expand(-1, geom.padded_patches).reshape(-1)
    m = pad[:, None] & pad[None, :]
    if has(mutant, "no_pad_mask"):
        m = torch.zeros_like(m)
    if has(mutant, "pad_keys_masked"):
        m = pad[None, :].expand(pad.numel(), -1).clone()
    if has(mutant, "tile_local"):
        tile = torch.arange(pad.numel()) // geom.padded_patches
        m = m | (tile[:, None] != tile[None, :])
    if has(mutant, "key_dropped"):
        m = m.clone()
        m[:, DROPPED_KEY] = True
    return m if bool(m.any()) else None


def _block(x, w, p, masked, geom, dtype, mutant=None, gates=None):
    """One block on x [T, D]; `gates` = (gate_attn, gate_ffn) of a global layer as the checkpoint holds them, None for a local one"""
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    t = lambda name: _t(w, p + name, dtype)  # noqa: E731
    l1, l2 = "input_layernorm", "post_attention_layernorm"
    if has(mutant, "ln_exchanged"):
        l1, l2 = l2, l1
    fa = ff = None  # the factor of a branch
    if gates is not None and not has(mutant, "gates_ignored"):
        ga, gf = gates[::-1] if has(mutant, "gates_exchanged") else gates
        fa, ff = (ga, gf) if has(mutant, "gate_without_tanh") else (math.tanh(ga), math.tanh(gf))
    h = _ln(x, t(l1 + ".weight"), t(l1 + ".bias"), geom.norm_eps)
    q = stored(h @ t("self_attn.q_proj.weight").T, mutant).reshape(-1, H, dh).transpose(0, 1)
    k = stored(h @ t("self_attn.k_proj.weight").T, mutant).reshape(-1, H, dh).transpose(0, 1)
    v = stored(h @ t("self_attn.v_proj.weight").T, mutant).reshape(-1, H, dh).transpose(0, 1)
    if has(mutant, "qk_exchanged"):
        q, k = k, q
    if has(mutant, "heads_rolled"):
        v = v.roll(1, dims=0)
    out = torch.empty_like(q)
    for hd in range(H):  # one head at a time, as the oracle
        s = q[hd] @ k[hd].T
        if not has(mutant, "no_q_scale"):
            s = s * dh ** -0.5
        if has(mutant, "uniform_attention"):
            s = torch.zeros_like(s)
        if masked is not None:
            s = s.masked_fill(masked, torch.finfo(torch.float32).min)
        out[hd] = torch.softmax(s, dim=-1) @ v[hd]
    a = stored(out.transpose(0, 1).reshape(-1, D), mutant) @ t("self_attn.o_proj.weight").T
    x = stored(x + (a if fa is None else fa * a), mutant)
    h = _ln(x, t(l2 + ".weight"), t(l2 + ".bias"), geom.norm_eps)
    h = torch.nn.functional.gelu(h @ t("mlp.fc1.weight").T + t("mlp.fc1.bias"), approximate="tanh" if has(mutant, "other_gelu") else "none")
    h = stored(h, mutant) @ t("mlp.fc2.weight").T + t("mlp.fc2.bias")
    h = h if ff is None else ff * h
    return stored(h if has(mutant, "no_mlp_residual") else x + h, mutant)


@torch.no_grad()
def local_state(pixel_values, aspect_ratio_id: int, num_tiles: int, w: dict, geom: TileViTGeometry = TILE_VIT, dtype=torch.float32, mutant=None):
    """The stem and the local layers: pixel_values f32 [max_tiles, 3, S, S] of ONE image -> (x [T * PP, D] behind the last local
    layer, the saved intermediate states), arithmetic in `dtype`"""
    D, T, NP, PP, P = geom.hidden_size, geom.max_num_tiles, geom.num_patches, geom.padded_patches, geom.patch_size
    t = lambda name: _t(w, name, dtype)  # noqa: E731
    px = torch.from_numpy(np.ascontiguousarray(pixel_values, dtype=np.float32)).to(dtype)
    g = geom.image_size // P
    patches = stored(px.reshape(T, geom.num_channels, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(T, g * g, geom.patch_dim), mutant)
    x = stored(patches @ t("patch_embedding.weight").reshape(D, -1).T, mutant)  # [T, 1600, D]
    pre = t("pre_tile_positional_embedding.embedding.weight")[aspect_ratio_id].reshape(T, 1, D) * _tanh_gate(w, "pre_tile_positional_embedding.gate")
    x = x + pre
    cls = t("class_embedding").expand(T, 1, D)
    if has(mutant, "pre_on_class"):
        cls = cls + pre
    x = torch.cat([cls, x], dim=1)  # [T, 1601, D]
    gp = _tanh_gate(w, "gated_positional_embedding.gate")
    x = x + (1.0 if has(mutant, "no_one_minus_gate") else 1.0 - gp) * t("gated_positional_embedding.embedding")[None]
    tile_emb = t("gated_positional_embedding.tile_embedding.weight")[aspect_ratio_id].reshape(T, NP, D)
    x = x + gp * (tile_emb.roll(1, dims=0) if has(mutant, "tile_emb_rolled") else tile_emb)
    if not has(mutant, "no_ln_pre"):
        x = _ln(x, t("layernorm_pre.weight"), t("layernorm_pre.bias"), 1e-5)
    x = torch.nn.functional.pad(stored(x, mutant), (0, 0, 0, PP - NP)).reshape(T * PP, D)
    masked = masked_pairs(num_tiles, geom, mutant)
    keep = []
    before = getattr(geom, "intermediate_save_point", "after") == "before"
    for i in range(geom.num_layers):
        if before and i in geom.intermediate_layers:
            keep.append(x)
        x = _block(x, w, f"transformer.layers.{i}.", masked, geom, dtype, mutant)
        if not before and i in geom.intermediate_layers:
            keep.append(x)
    return x, keep


@torch.no_grad()
def tile_states(pixel_values, aspect_ratio_id: int, num_tiles: int, w: dict, geom: TileViTGeometry = TILE_VIT, dtype=torch.float32,
                mutant=None, local=None):
    """-> (the final state [T, 1601, D], the saved intermediate states, each [T, 1601, D]).  `local`: what `local_state` returned
    for the same inputs and `dtype`, to spare the stem and the local layers (mutants of LOCAL_FREE only)."""
    D, T, NP, PP = geom.hidden_size, geom.max_num_tiles, geom.num_patches, geom.padded_patches
    t = lambda name: _t(w, name, dtype)  # noqa: E731
    if local is not None:
        names = {mutant} if isinstance(mutant, str) else set(mutant or ())
        assert names <= LOCAL_FREE, f"{names - LOCAL_FREE} change the stem or the local layers"
    x, keep = local if local is not None else local_state(pixel_values, aspect_ratio_id, num_tiles, w, geom, dtype, mutant)
    post = t("post_tile_positional_embedding.embedding.weight")[aspect_ratio_id].reshape(T, 1, D)
    post = post * _tanh_gate(w, "post_tile_positional_embedding.gate")
    if has(mutant, "post_emb_before_ln"):
        x = _ln(x.reshape(T, PP, D) + post, t("layernorm_post.weight"), t("layernorm_post.bias"), 1e-5).reshape(T * PP, D)
    else:
        if not has(mutant, "no_ln_post"):
            x = _ln(x, t("layernorm_post.weight"), t("layernorm_post.bias"), 1e-5)
        x = x.reshape(T, PP, D)
        x = (x if has(mutant, "no_post_emb") else x + post).reshape(T * PP, D)
    x = stored(x, mutant)
    masked = masked_pairs(num_tiles, geom, mutant)
    for i in range(geom.num_global_layers):
        p = f"global_transformer.layers.{i}."
        x = _block(x, w, p, masked, geom, dtype, mutant, (float(w[p + "gate_attn"][0]), float(w[p + "gate_ffn"][0])))
    return x.reshape(T, PP, D)[:, :NP], [s.reshape(T, PP, D)[:, :NP] for s in keep]


def vision_forward(pixel_values, aspect_ratio_id: int, num_tiles: int, w: dict, geom: TileViTGeometry = TILE_VIT, dtype=torch.float32,
                   mutant=None, local=None) -> np.ndarray:
    """-> last_hidden_state [max_tiles, 1601, D (1 + k)] in `dtype`: oracle.mllama_vision.vision_forward's output, feature D + d k + layer
    the saved state `layer` at dimension d"""
    final, keep = tile_states(pixel_values, aspect_ratio_id, num_tiles, w, geom, dtype, mutant, local)
    inter = torch.stack(keep, dim=-1).reshape(final.shape[0], final.shape[1], -1)
    return torch.cat([final, inter], dim=-1).numpy()


def split_row(hidden, geom: TileViTGeometry = TILE_VIT) -> dict:
    """[..., D (1 + k)] in the layout above -> {"final": [..., D], "intermediate <layer>": [..., D] per saved layer}, float64"""
    h = np.asarray(hidden, dtype=np.float64)
    D, k = geom.hidden_size, len(geom.intermediate_layers)
    assert h.shape[-1] == D * (1 + k)
    inter = h[..., D:].reshape(*h.shape[:-1], D, k)
    return {"final": h[..., :D], **{f"intermediate {layer}": inter[..., j] for j, layer in enumerate(geom.intermediate_layers)}}


def tile_outputs(pixel_values, aspect_ratio_id: int, num_tiles: int, w: dict, geom: TileViTGeometry = TILE_VIT, dtype=torch.float64,
                 mutant=None, local=None) -> dict:
    """name -> float64 [rows groups, rows, width] of every output the GPU test compares: the slices of `split_row` over all four tiles
    [4, 1601, D], and "pooled" [1, 1, D (1 + k)]: the whole row of the class token of tile 0 (oracle.mllama_vision.pooled_embedding;
    "pooled_tile_1": of tile 1), x / max(||x||, 1e-12)"""
    hidden = vision_forward(pixel_values, aspect_ratio_id, num_tiles, w, geom, dtype, mutant, local)
    out = split_row(hidden, geom)
    v = np.asarray(hidden[1 if has(mutant, "pooled_tile_1") else 0, 0], dtype=np.float64)
    out["pooled"] = (v / max(np.linalg.norm(v), 1e-12))[None, None, :]
    return out
