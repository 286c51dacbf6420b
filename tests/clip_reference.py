"""Test infrastructure: the CLIP ViT/16 image tower restated in plain torch (float32 or float64, CPU), from transformers 5.15.0
models/clip/modeling_clip.py.  What each step restates:

    :138-217  CLIPVisionEmbeddings      Conv2d(k = 16, s = 16, bias=False) (:148-154) -> flatten -> transpose; class_embedding
                                        prepended (:212-213); + position_embedding(position_ids) (:217)
    :642      CLIPVisionModel.forward   hidden_states = self.pre_layrnorm(hidden_states)      (LayerNorm, eps = layer_norm_eps, :605)
    :353-390  CLIPEncoderLayer          x + self_attn(layer_norm1(x)) (:370-377); x + mlp(layer_norm2(x)) (:379-381)
    :259-277  eager_attention_forward   softmax(q k^T * scaling) (:272, in f32) @ v, scaling = head_dim ** -0.5 (:289, :327);
                                        q / k / v / out projections with bias
    :338-350  CLIPMLP                   fc2(ACT2FN[hidden_act](fc1(x))) (:342, :348); "quick_gelu" is activations.py:117-123
                                        `input * torch.sigmoid(1.702 * input)`, "gelu" is erf-GELU
    :650-651  CLIPVisionModel.forward   pooled_output = self.post_layernorm(last_hidden_state[:, 0, :])
    :950      CLIPVisionModelWithProjection.forward   image_embeds = self.visual_projection(pooled_output)  (Linear, bias=False, :907)

`tests/golden/make_clip_golden.py` records what the two transformers classes themselves return on seeded weights and
inputs (tests/golden/clip_cases.npz); tests/test_clip_cpu.py holds this restatement to those rows.  The GPU tests compare the
engine with this restatement, pooled at any token (the classes pool token 0 only).

The bf16 helpers (`rne_bf16_bits`, `ulp_bf16`) are those of tests/test_gpu_gemm.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from multimodal_embeddings_amd.weights import CLIP_B16, CLIPGeometry
from test_gpu_gemm import rne_bf16_bits, ulp_bf16  # noqa: F401  (re-exported)


def _t(w, name, dtype):
    return torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dtype)


def layer_norm(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


ACT = {"quick_gelu": quick_gelu, "gelu": gelu_erf}


def patchify(pixel_values: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """[n, 3, H, W] -> [n, (H / patch)(W / patch), 3 patch patch], a row in (c, ky, kx) order: the Conv2d's receptive fields"""
    n, c, H, W = pixel_values.shape
    x = pixel_values.reshape(n, c, H // patch, patch, W // patch, patch)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(n, (H // patch) * (W // patch), c * patch * patch)


@torch.no_grad()
def clip_hidden_states(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32) -> torch.Tensor:
    """pixel_values [n, 3, 224, 224] -> last_hidden_state [n, 197, D] (before post_layernorm), arithmetic in `dtype`"""
    x = torch.as_tensor(np.asarray(pixel_values)).to(dtype)
    n = x.shape[0]
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    v = "vision_model."
    x = patchify(x, geom.patch_size) @ _t(w, v + "embeddings.patch_embedding.weight", dtype).reshape(D, -1).T  # no bias
    cls = _t(w, v + "embeddings.class_embedding", dtype).reshape(1, 1, D).expand(n, 1, D)
    x = torch.cat([cls, x], dim=1) + _t(w, v + "embeddings.position_embedding.weight", dtype).reshape(1, geom.seq_len, D)
    x = layer_norm(x, _t(w, v + "pre_layrnorm.weight", dtype), _t(w, v + "pre_layrnorm.bias", dtype), geom.layer_norm_eps)
    act = ACT[geom.hidden_act]
    for i in range(geom.num_layers):
        p = f"{v}encoder.layers.{i}."
        lin = lambda t, name: t @ _t(w, p + name + ".weight", dtype).T + _t(w, p + name + ".bias", dtype)  # noqa: E731
        h = layer_norm(x, _t(w, p + "layer_norm1.weight", dtype), _t(w, p + "layer_norm1.bias", dtype), geom.layer_norm_eps)
        q, k, val = (lin(h, f"self_attn.{m}_proj").view(n, -1, H, dh).transpose(1, 2) for m in "qkv")
        s = torch.softmax((q @ k.transpose(2, 3)) * (dh ** -0.5), dim=-1)
        x = x + lin((s @ val).transpose(1, 2).reshape(n, -1, D), "self_attn.out_proj")
        h = layer_norm(x, _t(w, p + "layer_norm2.weight", dtype), _t(w, p + "layer_norm2.bias", dtype), geom.layer_norm_eps)
        x = x + lin(act(lin(h, "mlp.fc1")), "mlp.fc2")
    return x


@torch.no_grad()
def clip_forward(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, tok: int = 0, batch: int = 8):
    """-> (pooler_output [n, D] = post_layernorm of token `tok`, image_embeds [n, P] or None without a projection), numpy in
    `dtype`, not normalised: what CLIPVisionModel / CLIPVisionModelWithProjection return (for tok = 0)."""
    v = "vision_model."
    pooled, proj = [], []
    pv = np.asarray(pixel_values)
    for s in range(0, pv.shape[0], batch):
        hs = clip_hidden_states(pv[s : s + batch], w, geom, dtype)
        po = layer_norm(hs[:, tok, :], _t(w, v + "post_layernorm.weight", dtype), _t(w, v + "post_layernorm.bias", dtype), geom.layer_norm_eps)
        pooled.append(po)
        if geom.projection_dim:
            proj.append(po @ _t(w, "visual_projection.weight", dtype).T)
    return torch.cat(pooled).numpy(), (torch.cat(proj).numpy() if proj else None)


def clip_embed(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, pool: str = "cls") -> np.ndarray:
    """The engine's contract: image_embeds (pooler_output without a projection) of the pooled token, x / max(||x||, 1e-12)"""
    pooled, proj = clip_forward(pixel_values, w, geom, dtype, tok={"cls": 0, "last": geom.seq_len - 1}[pool])
    e = proj if proj is not None else pooled
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
