"""Test infrastructure: the SigLIP ViT/16 image tower restated in plain torch (float32 or float64, CPU), from transformers
5.15.0 models/siglip/modeling_siglip.py.  What each step restates:

    SiglipVisionEmbeddings                  Conv2d(k = 16, s = 16, WITH bias) -> flatten -> transpose; + position_embedding; no class token
    SiglipEncoderLayer                      x + self_attn(layer_norm1(x)); x + mlp(layer_norm2(x)); eager attention
                                            softmax(q k^T * head_dim ** -0.5) @ v, q / k / v / out projections with bias
    SiglipMLP                               fc2(ACT2FN["gelu_pytorch_tanh"](fc1(x))): 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))
    SiglipVisionModel.forward               last_hidden_state = post_layernorm(every token row); pooler_output = head(last_hidden_state)
    SiglipMultiheadAttentionPoolingHead     a = MultiheadAttention(probe, h, h) (in_proj split q | k | v, heads of head_dim, out_proj with
                                            bias); y = a + mlp(layernorm(a)); return y[:, 0] -- the probe is no residual

`tests/golden/make_siglip_golden.py` records what `SiglipVisionModel` itself returns on seeded weights and inputs
(tests/golden/siglip_cases.npz); tests/test_siglip_cpu.py holds this restatement to those rows.  The GPU tests compare the
engine with this restatement.  `gelu_tanh_sigmoid` is the form the GEMM epilogue evaluates (csrc/gemm_epilogue.h).  `mutant=` switches
on one of the wrong towers of tests/tower_mutants.py (clip_reference.py holds the shared pieces); with None the arithmetic is the restatement's.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from clip_reference import block, block_getter, final_rows, gelu_erf, has, patch_rows, position_rows, stored
from multimodal_embeddings_amd.weights import CLIP_BLOCK, SIGLIP_B16, SiglipGeometry

V = "vision_model."
C0 = 2.0 * math.sqrt(2.0 / math.pi)
C1 = 0.044715 * C0


def _t(w, name, dtype):
    return torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dtype)


def layer_norm(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x**3)))


def gelu_tanh_sigmoid(x):
    """x * sigmoid(x (c0 + c1 x^2)), c0 = 2 sqrt(2 / pi), c1 = 0.044715 c0: the same function (0.5 (1 + tanh u) = sigmoid(2 u))"""
    return x * torch.sigmoid(x * (C0 + C1 * x * x))


def patchify(pixel_values: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """[n, 3, H, W] -> [n, (H / patch)(W / patch), 3 patch patch], a row in (c, ky, kx) order: the Conv2d's receptive fields"""
    n, c, H, W = pixel_values.shape
    x = pixel_values.reshape(n, c, H // patch, patch, W // patch, patch)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(n, (H // patch) * (W // patch), c * patch * patch)


@torch.no_grad()
def siglip_hidden_states(pixel_values, w: dict, geom: SiglipGeometry = SIGLIP_B16, dtype=torch.float32, mutant=None) -> torch.Tensor:
    """pixel_values [n, 3, 224, 224] -> the encoder's output [n, 196, D] (before post_layernorm), arithmetic in `dtype`.
    `mutant`: the switches of clip_reference.py ("other_gelu": erf-GELU)."""
    x = torch.as_tensor(np.asarray(pixel_values)).to(dtype)
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    x = patch_rows(x, geom.patch_size, mutant) @ _t(w, V + "embeddings.patch_embedding.weight", dtype).reshape(D, -1).T + _t(w, V + "embeddings.patch_embedding.bias", dtype)
    x = stored(x + position_rows(_t(w, V + "embeddings.position_embedding.weight", dtype), mutant).reshape(1, geom.seq_len, D), mutant)
    act = gelu_erf if has(mutant, "other_gelu") else gelu_tanh
    for i in range(geom.num_layers):
        x = block(x, block_getter(w, f"{V}encoder.layers.{i}.", CLIP_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant)
    return x


def _post_ln(w, dtype):
    return _t(w, V + "post_layernorm.weight", dtype), _t(w, V + "post_layernorm.bias", dtype)


@torch.no_grad()
def siglip_head(hs: torch.Tensor, w: dict, geom: SiglipGeometry = SIGLIP_B16, dtype=torch.float32, mutant=None) -> torch.Tensor:
    """The encoder's output [n, 196, D] -> pooler_output [n, D]: post_layernorm, then the attention-pooling head.
    Mutants of this step: "no_final_ln" / "kv_without_post_ln" (K | V read the encoder's output), "probe_unscaled" (no dh^-0.5),
    "mean_pooled_head" (uniform scores), "no_head_mlp_residual", and "other_gelu"."""
    n = hs.shape[0]
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    h = hs if has(mutant, "no_final_ln") or has(mutant, "kv_without_post_ln") else layer_norm(hs, *_post_ln(w, dtype), geom.layer_norm_eps)
    p = V + "head."
    wi, bi = _t(w, p + "attention.in_proj_weight", dtype), _t(w, p + "attention.in_proj_bias", dtype)
    probe = _t(w, p + "probe", dtype).reshape(1, D)
    q = (probe @ wi[:D].T + bi[:D]).view(1, 1, H, dh).transpose(1, 2)                 # [1, H, 1, dh], the same for every crop
    k = (h @ wi[D : 2 * D].T + bi[D : 2 * D]).view(n, -1, H, dh).transpose(1, 2)      # [n, H, 196, dh]
    val = (h @ wi[2 * D :].T + bi[2 * D :]).view(n, -1, H, dh).transpose(1, 2)
    s = (q @ k.transpose(2, 3)) * (1.0 if has(mutant, "probe_unscaled") else dh ** -0.5)
    s = torch.softmax(torch.zeros_like(s) if has(mutant, "mean_pooled_head") else s, dim=-1)  # [n, H, 1, 196]
    a = (s @ val).transpose(1, 2).reshape(n, D)
    a = a @ _t(w, p + "attention.out_proj.weight", dtype).T + _t(w, p + "attention.out_proj.bias", dtype)
    m = layer_norm(a, _t(w, p + "layernorm.weight", dtype), _t(w, p + "layernorm.bias", dtype), geom.layer_norm_eps)
    m = (gelu_erf if has(mutant, "other_gelu") else gelu_tanh)(m @ _t(w, p + "mlp.fc1.weight", dtype).T + _t(w, p + "mlp.fc1.bias", dtype))
    m = m @ _t(w, p + "mlp.fc2.weight", dtype).T + _t(w, p + "mlp.fc2.bias", dtype)
    return m if has(mutant, "no_head_mlp_residual") else a + m


@torch.no_grad()
def siglip_forward(pixel_values, w: dict, geom: SiglipGeometry = SIGLIP_B16, dtype=torch.float32, batch: int = 8, mutant=None) -> np.ndarray:
    """-> pooler_output [n, D], numpy in `dtype`, not normalised: what SiglipVisionModel returns"""
    pv = np.asarray(pixel_values)
    out = [siglip_head(siglip_hidden_states(pv[s : s + batch], w, geom, dtype, mutant), w, geom, dtype, mutant) for s in range(0, pv.shape[0], batch)]
    return torch.cat(out).numpy()


@torch.no_grad()
def siglip_token_rows(pixel_values, w: dict, geom: SiglipGeometry = SIGLIP_B16, dtype=torch.float64, mutant=None) -> np.ndarray:
    """-> [n, 196, D]: every token row behind post_layernorm, L2-normalised: what Engine.vit_tokens returns"""
    return final_rows(siglip_hidden_states(pixel_values, w, geom, dtype, mutant), *_post_ln(w, dtype), geom.layer_norm_eps, mutant).numpy()


def siglip_embed(pixel_values, w: dict, geom: SiglipGeometry = SIGLIP_B16, dtype=torch.float32, mutant=None) -> np.ndarray:
    """The engine's contract: pooler_output, x / max(||x||, 1e-12)"""
    e = siglip_forward(pixel_values, w, geom, dtype, mutant=mutant)
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
