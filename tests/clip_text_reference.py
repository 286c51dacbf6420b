"""Test infrastructure: the CLIP text tower restated in plain torch (float32 or float64, CPU), from transformers 5.15.0
models/clip/modeling_clip.py.  What each step restates:

    CLIPTextEmbeddings          token_embedding(input_ids) + position_embedding(position_ids), positions 0..76
    CLIPTextTransformer.forward a causal mask over the 77 positions (key j reaches query i only when j <= i); the padding
                                attention_mask the tokenizer returns is NOT needed for the pooled row: nothing behind the EOS
                                position reaches it
    CLIPEncoderLayer            x + self_attn(layer_norm1(x)); x + mlp(layer_norm2(x))
    eager_attention_forward     softmax(q k^T * head_dim ** -0.5 + mask) (in f32) @ v; q / k / v / out projections with bias
    CLIPMLP                     fc2(ACT2FN[hidden_act](fc1(x))): "quick_gelu" or erf "gelu"
    CLIPTextTransformer.forward last_hidden_state = final_layer_norm(...); pooled_output = the row at
                                  eos_token_id == 2:  input_ids.argmax(-1)                      (legacy configurations)
                                  otherwise:          (input_ids == eos_token_id).int().argmax(-1)   (the first such position)
    CLIPTextModelWithProjection text_embeds = text_projection(pooled_output)  (Linear, bias=False)

`tests/golden/make_clip_text_golden.py` records what the two transformers classes return on seeded weights and ids
(tests/golden/clip_text_cases.npz); tests/test_clip_text_cpu.py holds this restatement to those rows.  `mutant=` switches on one of the
wrong towers of tests/tower_mutants.py; with None the arithmetic is the restatement's.  `causal_attention_f64`
is the float64 attention the kernel test and the mutant test share, with the tolerance's scale A = sum p |v| / sum p.
"""
from __future__ import annotations

import numpy as np
import torch

from clip_reference import ACT, _t, block, block_getter, has, layer_norm, one_minus_cos, position_rows, stored  # noqa: F401  (re-exported)
from multimodal_embeddings_amd.weights import CLIP_BLOCK, CLIP_TEXT_B, CLIPTextGeometry

T = 77


def eos_positions(ids: np.ndarray, eos_token_id: int) -> np.ndarray:
    """transformers' rule; -1 where the first-occurrence rule finds nothing (transformers pools row 0 there, the engine refuses)"""
    ids = np.asarray(ids)
    if eos_token_id == 2:
        return ids.argmax(axis=1)
    hit = ids == eos_token_id
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


@torch.no_grad()
def clip_text_hidden_states(ids, w: dict, geom: CLIPTextGeometry = CLIP_TEXT_B, dtype=torch.float64, mutant=None) -> torch.Tensor:
    """ids [n, 77] -> the encoder's output [n, 77, D] (before final_layer_norm), arithmetic in `dtype`.
    `mutant`: the switches of clip_reference.py, and "no_causal_mask"."""
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
    D, H = geom.hidden_size, geom.num_heads
    dh = D // H
    t = "text_model."
    x = _t(w, t + "embeddings.token_embedding.weight", dtype)[ids] + position_rows(_t(w, t + "embeddings.position_embedding.weight", dtype), mutant).reshape(1, T, D)
    x = stored(x, mutant)
    mask = None if has(mutant, "no_causal_mask") else torch.full((T, T), float("-inf"), dtype=dtype).triu(1)
    act = ACT[geom.hidden_act]
    if has(mutant, "other_gelu"):
        act = ACT["gelu" if geom.hidden_act == "quick_gelu" else "quick_gelu"]
    for i in range(geom.num_layers):
        x = block(x, block_getter(w, f"{t}encoder.layers.{i}.", CLIP_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant, mask)
    return x


@torch.no_grad()
def clip_text_forward(ids, w: dict, geom: CLIPTextGeometry = CLIP_TEXT_B, dtype=torch.float64, batch: int = 16, mutant=None):
    """-> (pooler_output [n, D], text_embeds [n, P] or None without a projection), numpy in `dtype`, not normalised: what
    CLIPTextModel / CLIPTextModelWithProjection return.  Mutants of this step: "pooled_last" (position 76),
    "pooled_before_eos", "no_final_ln"."""
    ids = np.asarray(ids)
    pos = eos_positions(ids, geom.eos_token_id)
    assert (pos >= 0).all(), "a sequence holds no eos_token_id"
    if has(mutant, "pooled_last"):
        pos = np.full_like(pos, T - 1)
    if has(mutant, "pooled_before_eos"):
        pos = np.maximum(pos - 1, 0)
    t = "text_model."
    pooled, proj = [], []
    for s in range(0, ids.shape[0], batch):
        hs = clip_text_hidden_states(ids[s : s + batch], w, geom, dtype, mutant)
        rows = hs[torch.arange(hs.shape[0]), torch.as_tensor(pos[s : s + batch])]
        po = rows if has(mutant, "no_final_ln") else layer_norm(rows, _t(w, t + "final_layer_norm.weight", dtype),
                                                                _t(w, t + "final_layer_norm.bias", dtype), geom.layer_norm_eps)
        pooled.append(po)
        if geom.projection_dim:
            proj.append(po @ _t(w, "text_projection.weight", dtype).T)
    return torch.cat(pooled).numpy(), (torch.cat(proj).numpy() if proj else None)


def clip_text_embed(ids, w: dict, geom: CLIPTextGeometry = CLIP_TEXT_B, dtype=torch.float64, mutant=None) -> np.ndarray:
    """The engine's contract: text_embeds (pooler_output without a projection), x / max(||x||, 1e-12)"""
    pooled, proj = clip_text_forward(ids, w, geom, dtype, mutant=mutant)
    e = proj if proj is not None else pooled
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


# ---- the attention kernel's contract in float64 ---------------------------------------------------------------------------
SC = float(np.float32(0.125) * np.float32(1.44269504088896341))  # dh^-0.5 log2 e as the loaders fold it into the query rows


def planted_qkv(n: int, heads: int, seed: int = 0, q_scale: float = 2.0) -> np.ndarray:
    """bf16-representable f32 [n * 77, 3 * 64 * heads] Q | K | V; Q in the log2 units the kernel takes (already scaled), wide
    enough that the softmax is far from uniform"""
    from multimodal_embeddings_amd.weights import irwin_hall_normal, round_to_bf16

    D = 64 * heads
    z = irwin_hall_normal(seed, 0x7200 + heads, n * T * 3 * D).reshape(n * T, 3 * D)
    z[:, :D] *= np.float32(q_scale * SC)
    return round_to_bf16(z).reshape(n * T, 3 * D)


def causal_attention_f64(qkv: np.ndarray, n: int, heads: int, *, allowed=None, q_factor: float = 1.0, keys: int = T):
    """float64 attention over pre-scaled Q (log2 units): out [n * 77, 64 * heads], A [n * 77, 64 * heads] = sum p |v| / sum p.
    `allowed` [77, keys] bool (default: the causal mask j <= i) and `q_factor` / `keys` exist for the mutant test: a wrong
    mask, a missing scale, and padded keys 77.. that hold copies of row 76 (what the kernel's clamped LDS rows hold)."""
    D = 64 * heads
    x = np.asarray(qkv, dtype=np.float64).reshape(n, T, 3, heads, 64)
    q, k, v = x[:, :, 0].transpose(0, 2, 1, 3) * q_factor, x[:, :, 1].transpose(0, 2, 1, 3), x[:, :, 2].transpose(0, 2, 1, 3)
    if keys > T:
        pad = keys - T
        k = np.concatenate([k, np.repeat(k[:, :, -1:], pad, axis=2)], axis=2)
        v = np.concatenate([v, np.repeat(v[:, :, -1:], pad, axis=2)], axis=2)
    if allowed is None:
        allowed = np.tril(np.ones((T, keys), dtype=bool))
    s = np.where(allowed[None, None], q @ k.transpose(0, 1, 3, 2), -np.inf)
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    den = p.sum(axis=-1, keepdims=True)
    out = (p @ v) / den
    A = (p @ np.abs(v)) / den
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(n * T, D)  # noqa: E731
    return back(out), back(A)


def attention_tolerance(ref: np.ndarray, A: np.ndarray) -> np.ndarray:
    """|got - ref| <= 2^-8 |ref| + 2^-8 A: the bound tests/test_gpu_attention.py derives for P rounded to bf16 before P . V and
    the output rounded to bf16"""
    return 2.0 ** -8 * np.abs(ref) + 2.0 ** -8 * A
