"""Test infrastructure: the DINOv2 ViT/14 image tower restated in plain torch (float32 or float64, CPU), from transformers
5.15.0 models/dinov2/modeling_dinov2.py.  What each step restates:

    Dinov2PatchEmbeddings               Conv2d(k = 14, s = 14, WITH bias) -> flatten -> transpose: 256 patches at 224 pixels
    Dinov2Embeddings                    cat(cls_token, patches) + interpolate_pos_encoding: the [1, 1 + g * g, D] table with its class
                                        row kept and its g x g patch grid brought to 16 x 16 by F.interpolate(f32, bicubic,
                                        align_corners = False) (a 257-row table is returned as it is); mask_token is not read
    Dinov2Layer                         x + lambda1 * attention(norm1(x)); x + lambda2 * mlp(norm2(x)); eager attention
                                        softmax(q k^T * head_dim ** -0.5) @ v, query / key / value / output.dense with bias
    Dinov2MLP                           fc2(gelu(fc1(x))), erf-GELU
    Dinov2Model.forward                 sequence_output = layernorm(every token row); pooler_output = sequence_output[:, 0]

`tests/golden/make_dinov2_golden.py` records what `Dinov2Model` itself returns on seeded weights and inputs
(tests/golden/dinov2_cases.npz); tests/test_dinov2_cpu.py holds this restatement to those rows.  The GPU tests compare the
engine with this restatement.  `mutate=` names the two wrong models tests/test_gpu_dinov2.py asks for; `mutant=` switches on one
of the wrong towers of tests/tower_mutants.py (clip_reference.py holds the shared pieces); with neither the arithmetic is the restatement's.
"""
from __future__ import annotations

import numpy as np
import torch

from clip_reference import block, block_getter, final_rows, has, neighbour, patch_rows, position_rows, stored
from multimodal_embeddings_amd.weights import DINOV2_B14, DINOV2_BLOCK, Dinov2Geometry
from siglip_reference import gelu_tanh

POS = "embeddings.position_embeddings"


def _t(w, name, dtype):
    return torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dtype)


def layer_norm(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (2.0 ** -0.5)))


def patchify(pixel_values: torch.Tensor, patch: int = 14) -> torch.Tensor:
    """[n, 3, H, W] -> [n, (H / patch)(W / patch), 3 patch patch], a row in (c, ky, kx) order: the Conv2d's receptive fields"""
    n, c, H, W = pixel_values.shape
    x = pixel_values.reshape(n, c, H // patch, patch, W // patch, patch)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(n, (H // patch) * (W // patch), c * patch * patch)


def position_table(w: dict, dtype=torch.float32) -> torch.Tensor:
    """-> [257, D] in `dtype`: the interpolation itself always runs in float32, as the model's does"""
    t = _t(w, POS, torch.float32).reshape(-1, np.shape(w[POS])[-1])
    g = int(round((t.shape[0] - 1) ** 0.5))
    if g == 16:
        return t.to(dtype)
    D = t.shape[1]
    patch = torch.nn.functional.interpolate(t[1:].reshape(1, g, g, D).permute(0, 3, 1, 2), size=(16, 16), mode="bicubic", align_corners=False)
    return torch.cat((t[:1], patch.permute(0, 2, 3, 1).reshape(256, D)), dim=0).to(dtype)


@torch.no_grad()
def dinov2_hidden_states(pixel_values, w: dict, geom: Dinov2Geometry = DINOV2_B14, dtype=torch.float32, mutate: str | None = None,
                         mutant=None) -> torch.Tensor:
    """pixel_values [n, 3, 224, 224] -> the encoder's output [n, 257, D] (before the final layernorm), arithmetic in `dtype`.
    mutate: "swap_pos" exchanges the position rows 1 and 2, "no_layer_scale2" leaves layer_scale2 out of every block.
    mutant: the switches of clip_reference.py, and of this tower "no_layer_scale" (both scales left out), "ls_exchanged"
    (lambda2 behind the attention, lambda1 behind the MLP), "cls_pos_from_grid" (the class token gets the first row of the
    interpolated patch grid instead of the table's class row), "other_gelu" (tanh-GELU)."""
    x = torch.as_tensor(np.asarray(pixel_values)).to(dtype)
    n = x.shape[0]
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    x = patch_rows(x, geom.patch_size, mutant) @ _t(w, "embeddings.patch_embeddings.projection.weight", dtype).reshape(D, -1).T
    x = x + _t(w, "embeddings.patch_embeddings.projection.bias", dtype)
    x = torch.cat((_t(w, "embeddings.cls_token", dtype).reshape(1, 1, D).expand(n, 1, D), x), dim=1)
    pos = position_table(w, dtype)
    if mutate == "swap_pos":
        pos = pos.clone()
        pos[[1, 2]] = pos[[2, 1]]
    if has(mutant, "cls_pos_from_grid"):
        pos = pos.clone()
        pos[0] = pos[1]
    x = stored(x + position_rows(pos, mutant).reshape(1, 257, D), mutant)
    act = gelu_tanh if has(mutant, "other_gelu") else gelu
    for i in range(geom.num_layers):
        p = f"encoder.layer.{i}."
        s1, s2 = _t(w, p + "layer_scale1.lambda1", dtype), _t(w, p + "layer_scale2.lambda1", dtype)
        if has(mutant, "ls_exchanged"):
            s1, s2 = s2, s1
        if has(mutant, "no_layer_scale"):
            s1 = s2 = None
        if mutate == "no_layer_scale2":
            s2 = None
        x = block(x, block_getter(w, p, DINOV2_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant, scale1=s1, scale2=s2)
    return x


def _final_ln(w, dtype):
    return _t(w, "layernorm.weight", dtype), _t(w, "layernorm.bias", dtype)


@torch.no_grad()
def dinov2_pool(hs, w: dict, geom: Dinov2Geometry = DINOV2_B14, dtype=torch.float32, token: int = 0, mutant=None) -> torch.Tensor:
    """The encoder's output [n, 257, D] -> layernorm(row `token`) [n, D]"""
    if has(mutant, "neighbour_pooled"):
        token = neighbour(token, 257)
    return hs[:, token] if has(mutant, "no_final_ln") else layer_norm(hs[:, token], *_final_ln(w, dtype), geom.layer_norm_eps)


@torch.no_grad()
def dinov2_forward(pixel_values, w: dict, geom: Dinov2Geometry = DINOV2_B14, dtype=torch.float32, batch: int = 8, token: int = 0,
                   mutate: str | None = None, mutant=None) -> np.ndarray:
    """-> layernorm(row `token`) [n, D], numpy in `dtype`, not normalised: token 0 is what Dinov2Model returns as pooler_output.
    Mutants of this step: "neighbour_pooled", "no_final_ln"."""
    pv = np.asarray(pixel_values)
    out = [dinov2_pool(dinov2_hidden_states(pv[s : s + batch], w, geom, dtype, mutate, mutant), w, geom, dtype, token, mutant)
           for s in range(0, pv.shape[0], batch)]
    return torch.cat(out).numpy()


@torch.no_grad()
def dinov2_token_rows(pixel_values, w: dict, geom: Dinov2Geometry = DINOV2_B14, dtype=torch.float64, mutant=None) -> np.ndarray:
    """-> [n, 257, D]: every token row behind the final layernorm, L2-normalised: what Engine.vit_tokens returns"""
    return final_rows(dinov2_hidden_states(pixel_values, w, geom, dtype, None, mutant), *_final_ln(w, dtype), geom.layer_norm_eps, mutant).numpy()


def dinov2_embed(pixel_values, w: dict, geom: Dinov2Geometry = DINOV2_B14, dtype=torch.float32, token: int = 0, mutant=None) -> np.ndarray:
    """The engine's contract: the pooled row, x / max(||x||, 1e-12)"""
    e = dinov2_forward(pixel_values, w, geom, dtype, token=token, mutant=mutant)
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


def retile_p14_reference(patches16: np.ndarray) -> np.ndarray:
    """What retile_patches_p14 (csrc/dinov2.hip) computes, in numpy: K1's patch-16 matrix [n * 196, 768] (any dtype) -> the
    patch-14 matrix [n * 256, 640], conv order (c, ky, kx), columns 588..639 zero."""
    p = np.asarray(patches16)
    n = p.shape[0] // 196
    dst = np.zeros((n * 256, 640), dtype=p.dtype)
    P = np.arange(256)
    col = np.arange(588)
    c, ky, kx = col // 196, (col % 196) // 14, col % 14
    y = 14 * (P // 16)[:, None] + ky[None, :]
    x = 14 * (P % 16)[:, None] + kx[None, :]
    srow = (y // 16) * 14 + x // 16
    scol = c[None, :] * 256 + (y % 16) * 16 + x % 16
    src = p.reshape(n, 196, 768)
    dst.reshape(n, 256, 640)[:, :, :588] = src[:, srow, scol]
    return dst


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
