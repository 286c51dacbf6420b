"""Test infrastructure: the SigLIP text tower restated in plain torch (float32 or float64, CPU), from transformers 5.15.0
models/siglip/modeling_siglip.py.  What each step restates:

    SiglipTextEmbeddings          token_embedding(input_ids) + position_embedding(position_ids), positions 0..63
    SiglipEncoder                 pre-LN blocks with NO mask of any kind: no attention_mask is passed (the model was trained on
                                  padding="max_length"), so pad tokens are attended
    SiglipEncoderLayer            x + self_attn(layer_norm1(x)); x + mlp(layer_norm2(x))
    eager_attention_forward       softmax(q k^T * head_dim ** -0.5) (in f32) @ v; q / k / v / out projections with bias
    SiglipMLP                     fc2(gelu_pytorch_tanh(fc1(x)))
    SiglipTextTransformer.forward last_hidden_state = final_layer_norm(...); pooled = last_hidden_state[:, -1, :] -- the row at
                                  position 63, padding or not; pooler_output = head(pooled), a Linear WITH bias
    SiglipModel.forward           logits_per_text = cos(text, image) * exp(logit_scale) + logit_bias  (lines 798-805)

`tests/golden/make_siglip_text_golden.py` records what SiglipTextModel / SiglipModel return on seeded weights and ids
(tests/golden/siglip_text_cases.npz); tests/test_siglip_text_cpu.py holds this restatement to those rows.  The keyword switches
of `siglip_text_forward` (`pool_pos`, `causal`, `head_bias`) exist for the mutant tests, as does `mutant=` (tests/tower_mutants.py).  `attention_f64` is the float64 attention
the kernel test uses, with the tolerance's scale A = sum p |v| / sum p.
"""
from __future__ import annotations

import numpy as np
import torch

from clip_reference import _t, block, block_getter, gelu_erf, has, layer_norm, one_minus_cos, position_rows, stored  # noqa: F401  (re-exported)
from multimodal_embeddings_amd.weights import CLIP_BLOCK, SIGLIP_TEXT_B, SiglipTextGeometry

T = 64


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))


@torch.no_grad()
def siglip_text_hidden_states(ids, w: dict, geom: SiglipTextGeometry = SIGLIP_TEXT_B, dtype=torch.float64, causal: bool = False,
                              mutant=None) -> torch.Tensor:
    """ids [n, 64] -> the encoder's output [n, 64, D] (before final_layer_norm), arithmetic in `dtype`; `causal`: the mutant.
    `mutant`: the switches of clip_reference.py, "padding_masked" (no key at a pad_token_id position is attended) and
    "other_gelu" (erf-GELU)."""
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64))
    D, H = geom.hidden_size, geom.num_heads
    dh = D // H
    t = "text_model."
    x = _t(w, t + "embeddings.token_embedding.weight", dtype)[ids] + position_rows(_t(w, t + "embeddings.position_embedding.weight", dtype), mutant).reshape(1, T, D)
    x = stored(x, mutant)
    mask = torch.full((T, T), float("-inf"), dtype=dtype).triu(1) if causal else torch.zeros((T, T), dtype=dtype)
    if has(mutant, "padding_masked"):
        mask = mask + torch.where(ids == geom.pad_token_id, float("-inf"), 0.0).to(dtype).reshape(-1, 1, 1, T)
    act = gelu_erf if has(mutant, "other_gelu") else gelu_tanh
    for i in range(geom.num_layers):
        x = block(x, block_getter(w, f"{t}encoder.layers.{i}.", CLIP_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant, mask)
    return x


@torch.no_grad()
def siglip_text_forward(ids, w: dict, geom: SiglipTextGeometry = SIGLIP_TEXT_B, dtype=torch.float64, batch: int = 16, *, pool_pos: int = T - 1,
                        causal: bool = False, head_bias: bool = True, mutant=None) -> np.ndarray:
    """-> pooler_output [n, P], numpy in `dtype`, not normalised: what SiglipTextModel returns.  The keywords are the mutants;
    `mutant` names them too: "pooled_62", "no_head_bias", "no_final_ln"."""
    ids = np.asarray(ids)
    t = "text_model."
    if has(mutant, "pooled_62"):
        pool_pos = T - 2
    head_bias = head_bias and not has(mutant, "no_head_bias")
    out = []
    for s in range(0, ids.shape[0], batch):
        hs = siglip_text_hidden_states(ids[s : s + batch], w, geom, dtype, causal, mutant)
        po = hs[:, pool_pos] if has(mutant, "no_final_ln") else layer_norm(hs[:, pool_pos], _t(w, t + "final_layer_norm.weight", dtype),
                                                                          _t(w, t + "final_layer_norm.bias", dtype), geom.layer_norm_eps)
        y = po @ _t(w, t + "head.weight", dtype).T
        out.append(y + _t(w, t + "head.bias", dtype) if head_bias else y)
    return torch.cat(out).numpy()


def siglip_text_embed(ids, w: dict, geom: SiglipTextGeometry = SIGLIP_TEXT_B, dtype=torch.float64, **mutant) -> np.ndarray:
    """The engine's contract: pooler_output, x / max(||x||, 1e-12)"""
    e = siglip_text_forward(ids, w, geom, dtype, **mutant)
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


def siglip_logits_f64(text_unit: np.ndarray, image_unit: np.ndarray, logit_scale: float, logit_bias: float) -> np.ndarray:
    """SiglipModel.forward's logits_per_text [m, N] in float64 for unit rows"""
    return np.asarray(text_unit, np.float64) @ np.asarray(image_unit, np.float64).T * np.exp(np.float64(logit_scale)) + np.float64(logit_bias)


def sigmoid_f64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---- the attention kernel's contract in float64 ---------------------------------------------------------------------------
SC = float(np.float32(0.125) * np.float32(1.44269504088896341))  # dh^-0.5 log2 e as the loaders fold it into the query rows


def planted_qkv(n: int, heads: int, seed: int = 0, q_scale: float = 2.0) -> np.ndarray:
    """bf16-representable f32 [n * 64, 3 * 64 * heads] Q | K | V; Q in the log2 units the kernel takes (already scaled), wide
    enough that the softmax is far from uniform"""
    from multimodal_embeddings_amd.weights import irwin_hall_normal, round_to_bf16

    D = 64 * heads
    z = irwin_hall_normal(seed, 0x7300 + heads, n * T * 3 * D).reshape(n * T, 3 * D)
    z[:, :D] *= np.float32(q_scale * SC)
    return round_to_bf16(z).reshape(n * T, 3 * D)


def attention_f64(qkv: np.ndarray, n: int, heads: int):
    """float64 attention without a mask over pre-scaled Q (log2 units): out [n * 64, 64 * heads], A = sum p |v| / sum p"""
    D = 64 * heads
    x = np.asarray(qkv, dtype=np.float64).reshape(n, T, 3, heads, 64)
    q, k, v = x[:, :, 0].transpose(0, 2, 1, 3), x[:, :, 1].transpose(0, 2, 1, 3), x[:, :, 2].transpose(0, 2, 1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        s = q @ k.transpose(0, 1, 3, 2)
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
