"""Test infrastructure: the plain ViT tower (oracle/vit.py) with the mutant switches of tests/clip_reference.py and a choice of
`dtype`.  oracle/vit.py stays what tests/test_oracle_pins.py pins to transformers; tests/test_tower_sharpness_cpu.py holds this
file to it bit for bit in float32 with `mutant=None`.  It takes pixel values as the other restatements do (ViT/16 and ViT/32).
"""
from __future__ import annotations

import numpy as np
import torch

from clip_reference import (_t, block, block_getter, final_rows, gelu_erf, has, layer_norm, neighbour, patch_rows, position_rows,
                            stored)
from multimodal_embeddings_amd.weights import VIT_B16, VIT_BLOCK, ViTGeometry
from siglip_reference import gelu_tanh


@torch.no_grad()
def vit_hidden_states(pixel_values, w: dict, geom: ViTGeometry = VIT_B16, dtype=torch.float32, mutant=None) -> torch.Tensor:
    """pixel_values [n, 3, 224, 224] -> the encoder's output [n, T, D] (before the final layernorm), arithmetic in `dtype`;
    "other_gelu": tanh-GELU"""
    x = torch.as_tensor(np.asarray(pixel_values)).to(dtype)
    n = x.shape[0]
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    x = patch_rows(x, geom.patch_size, mutant) @ _t(w, "embeddings.patch_embeddings.projection.weight", dtype).reshape(D, -1).T
    x = x + _t(w, "embeddings.patch_embeddings.projection.bias", dtype)
    cls = _t(w, "embeddings.cls_token", dtype).reshape(1, 1, D).expand(n, 1, D)
    pos = position_rows(_t(w, "embeddings.position_embeddings", dtype).reshape(geom.seq_len, D), mutant)
    x = stored(torch.cat([cls, x], dim=1) + pos.reshape(1, geom.seq_len, D), mutant)
    act = gelu_tanh if has(mutant, "other_gelu") else gelu_erf
    for i in range(geom.num_layers):
        x = block(x, block_getter(w, f"layers.{i}.", VIT_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant)
    return x


def _final_ln(w, dtype):
    return _t(w, "layernorm.weight", dtype), _t(w, "layernorm.bias", dtype)


@torch.no_grad()
def vit_pool(hs, w: dict, geom: ViTGeometry = VIT_B16, dtype=torch.float32, token: int = 0, mutant=None) -> torch.Tensor:
    """The encoder's output [n, T, D] -> layernorm(row `token`) [n, D]; mutants of this step: "neighbour_pooled", "no_final_ln" """
    if has(mutant, "neighbour_pooled"):
        token = neighbour(token, geom.seq_len)
    return hs[:, token] if has(mutant, "no_final_ln") else layer_norm(hs[:, token], *_final_ln(w, dtype), geom.layer_norm_eps)


@torch.no_grad()
def vit_forward(pixel_values, w: dict, geom: ViTGeometry = VIT_B16, dtype=torch.float32, token: int = 0, mutant=None) -> np.ndarray:
    """-> layernorm(row `token`) [n, D], numpy in `dtype`, not normalised"""
    return vit_pool(vit_hidden_states(pixel_values, w, geom, dtype, mutant), w, geom, dtype, token, mutant).numpy()


@torch.no_grad()
def vit_token_rows(pixel_values, w: dict, geom: ViTGeometry = VIT_B16, dtype=torch.float64, mutant=None) -> np.ndarray:
    """-> [n, T, D]: every token row behind the final layernorm, L2-normalised: what Engine.vit_tokens returns"""
    return final_rows(vit_hidden_states(pixel_values, w, geom, dtype, mutant), *_final_ln(w, dtype), geom.layer_norm_eps, mutant).numpy()
