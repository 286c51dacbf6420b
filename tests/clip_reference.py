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
engine with this restatement, pooled at any token (the classes pool token 0 only).  `mutant=` switches on one of the wrong
towers of tests/tower_mutants.py (the helpers below are shared by all restatements); with None the arithmetic is the restatement's.

The bf16 helpers (`rne_bf16_bits`, `ulp_bf16`) are those of tests/test_gpu_gemm.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from multimodal_embeddings_amd.weights import CLIP_B16, CLIP_BLOCK, LAYER_FIELDS, CLIPGeometry
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


# ---- what the sharpness tests switch (tests/tower_mutants.py) ---------------------------------------------------------------
# `mutant` is None (the restatement: every function below then computes what it always did, operation for operation), one
# name, or a collection of names.  "bf16" is no wrong tower but the yardstick of tests/test_tower_sharpness_cpu.py: values
# rounded to bf16 where the engine stores bf16.  The helpers are shared by the five restatements and tests/vit_reference.py.
def has(mutant, name: str) -> bool:
    return mutant is not None and (mutant == name if isinstance(mutant, str) else name in mutant)


def stored(x: torch.Tensor, mutant) -> torch.Tensor:
    """x as the engine keeps it in memory under "bf16": rounded to nearest even; otherwise x itself"""
    return x.to(torch.bfloat16).to(x.dtype) if has(mutant, "bf16") else x


def patch_rows(x: torch.Tensor, patch: int, mutant=None) -> torch.Tensor:
    """patchify; "patch_kykxc": a row in (ky, kx, c) order, the pixel-interleaved layout of the crop itself"""
    p = patchify(x, patch)
    if has(mutant, "patch_kykxc"):
        p = p.reshape(p.shape[0], p.shape[1], 3, patch * patch).transpose(2, 3).reshape(p.shape)
    return stored(p, mutant)


def position_rows(pos: torch.Tensor, mutant=None) -> torch.Tensor:
    """The [T, D] position table; "pos_rolled": row t - 1 at token t; "first_row_without_pos": token 0 gets none"""
    if has(mutant, "pos_rolled"):
        pos = pos.roll(1, dims=0)
    if has(mutant, "first_row_without_pos"):
        pos = pos.clone()
        pos[0] = 0
    return pos


def attention(q, k, val, dh: int, mutant=None, mask=None):
    """softmax(q k^T dh^-0.5 [+ mask]) v on [n, H, T, dh]"""
    if has(mutant, "qk_exchanged"):
        q, k = k, q
    s = q @ k.transpose(2, 3)
    if not has(mutant, "no_q_scale"):
        s = s * (dh ** -0.5)
    if mask is not None:
        s = s + mask
    if has(mutant, "uniform_attention"):
        s = torch.where(torch.isinf(s), s, torch.zeros_like(s))
    if has(mutant, "last_key_dropped"):
        s = s.clone()
        s[..., -1] = float("-inf")
    if has(mutant, "first_key_dropped"):
        s = s.clone()
        s[..., 0] = float("-inf")
    s = torch.softmax(s, dim=-1)
    if has(mutant, "heads_rolled"):
        val = val.roll(1, dims=1)
    return s @ val


def block(x, get, H: int, dh: int, eps: float, act, mutant=None, mask=None, scale1=None, scale2=None):
    """One pre-LN block on x [n, T, D]: x + [scale1] out(attention(ln1(x))); x + [scale2] fc2(act(fc1(ln2(x)))).  `get(field)`
    gives the tensor of a weights.LAYER_FIELDS field; scale1 / scale2 are DINOv2's LayerScale."""
    n, D = x.shape[0], H * dh
    lin = lambda t, m: t @ get(m + "_w").T + get(m + "_b")  # noqa: E731
    l1, l2 = ("ln2", "ln1") if has(mutant, "ln_exchanged") else ("ln1", "ln2")
    h = layer_norm(x, get(l1 + "_g"), get(l1 + "_b"), eps)
    q, k, val = (stored(lin(h, m), mutant).view(n, -1, H, dh).transpose(1, 2) for m in "qkv")
    a = lin(stored(attention(q, k, val, dh, mutant, mask).transpose(1, 2).reshape(n, -1, D), mutant), "o")
    x = stored(x + (a if scale1 is None else a * scale1), mutant)
    h = layer_norm(x, get(l2 + "_g"), get(l2 + "_b"), eps)
    m = lin(stored(act(lin(h, "fc1")), mutant), "fc2")
    m = m if scale2 is None else m * scale2
    return stored(m if has(mutant, "no_mlp_residual") else x + m, mutant)


def block_getter(w: dict, prefix: str, names, dtype):
    """get(field) of `block` for the layer at `prefix`; `names`: a weights.*_BLOCK spelling"""
    by_field = dict(zip(LAYER_FIELDS, names))
    return lambda field: _t(w, prefix + by_field[field], dtype)


def neighbour(tok: int, T: int) -> int:
    """The token "neighbour_pooled" reads for `tok`: the next one, and the one before for the last"""
    return tok + 1 if tok + 1 < T else tok - 1


def final_rows(hs, g, b, eps: float, mutant=None) -> torch.Tensor:
    """Every row of hs [n, T, D] behind the tower's final LayerNorm, x / max(||x||, 1e-12): what Engine.vit_tokens returns.
    "no_final_ln" leaves the LayerNorm out, "neighbour_pooled" gives row neighbour(t) for t."""
    y = hs if has(mutant, "no_final_ln") else layer_norm(hs, g, b, eps)
    if has(mutant, "neighbour_pooled"):
        y = y[:, [neighbour(t, y.shape[1]) for t in range(y.shape[1])]]
    return y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)


@torch.no_grad()
def clip_hidden_states(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, mutant=None) -> torch.Tensor:
    """pixel_values [n, 3, 224, 224] -> last_hidden_state [n, 197, D] (before post_layernorm), arithmetic in `dtype`"""
    x = torch.as_tensor(np.asarray(pixel_values)).to(dtype)
    n = x.shape[0]
    D, H, dh = geom.hidden_size, geom.num_heads, geom.head_dim
    v = "vision_model."
    x = patch_rows(x, geom.patch_size, mutant) @ _t(w, v + "embeddings.patch_embedding.weight", dtype).reshape(D, -1).T  # no bias
    cls = _t(w, v + "embeddings.class_embedding", dtype).reshape(1, 1, D).expand(n, 1, D)
    x = torch.cat([cls, x], dim=1) + position_rows(_t(w, v + "embeddings.position_embedding.weight", dtype), mutant).reshape(1, geom.seq_len, D)
    x = stored(x, mutant)
    if not has(mutant, "no_pre_ln"):
        x = stored(layer_norm(x, _t(w, v + "pre_layrnorm.weight", dtype), _t(w, v + "pre_layrnorm.bias", dtype), geom.layer_norm_eps), mutant)
    act = ACT[geom.hidden_act]
    if has(mutant, "other_gelu"):
        act = ACT["gelu" if geom.hidden_act == "quick_gelu" else "quick_gelu"]
    for i in range(geom.num_layers):
        x = block(x, block_getter(w, f"{v}encoder.layers.{i}.", CLIP_BLOCK, dtype), H, dh, geom.layer_norm_eps, act, mutant)
    return x


def _post_ln(w, dtype):
    return _t(w, "vision_model.post_layernorm.weight", dtype), _t(w, "vision_model.post_layernorm.bias", dtype)


@torch.no_grad()
def clip_pool(hs, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, tok: int = 0, mutant=None):
    """last_hidden_state [n, 197, D] -> (pooler_output [n, D], image_embeds [n, P] or None) of token `tok`.  Mutants of this
    step: "neighbour_pooled", "no_final_ln", and "proj_before_post_ln": image_embeds = LayerNorm(projection(row)) with the first
    P of post_layernorm's parameters."""
    if has(mutant, "neighbour_pooled"):
        tok = neighbour(tok, geom.seq_len)
    g, b = _post_ln(w, dtype)
    po = hs[:, tok, :] if has(mutant, "no_final_ln") else layer_norm(hs[:, tok, :], g, b, geom.layer_norm_eps)
    if not geom.projection_dim:
        return po, None
    if has(mutant, "proj_before_post_ln"):
        P = geom.projection_dim
        return po, layer_norm(hs[:, tok, :] @ _t(w, "visual_projection.weight", dtype).T, g[:P], b[:P], geom.layer_norm_eps)
    return po, po @ _t(w, "visual_projection.weight", dtype).T


@torch.no_grad()
def clip_forward(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, tok: int = 0, batch: int = 8, mutant=None):
    """-> (pooler_output [n, D] = post_layernorm of token `tok`, image_embeds [n, P] or None without a projection), numpy in
    `dtype`, not normalised: what CLIPVisionModel / CLIPVisionModelWithProjection return (for tok = 0)."""
    pooled, proj = [], []
    pv = np.asarray(pixel_values)
    for s in range(0, pv.shape[0], batch):
        po, pr = clip_pool(clip_hidden_states(pv[s : s + batch], w, geom, dtype, mutant), w, geom, dtype, tok, mutant)
        pooled.append(po)
        if pr is not None:
            proj.append(pr)
    return torch.cat(pooled).numpy(), (torch.cat(proj).numpy() if proj else None)


@torch.no_grad()
def clip_token_rows(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float64, mutant=None) -> np.ndarray:
    """-> [n, 197, D]: every token row behind post_layernorm, L2-normalised: what Engine.vit_tokens returns"""
    return final_rows(clip_hidden_states(pixel_values, w, geom, dtype, mutant), *_post_ln(w, dtype), geom.layer_norm_eps, mutant).numpy()


def clip_embed(pixel_values, w: dict, geom: CLIPGeometry = CLIP_B16, dtype=torch.float32, pool: str = "cls", mutant=None) -> np.ndarray:
    """The engine's contract: image_embeds (pooler_output without a projection) of the pooled token, x / max(||x||, 1e-12)"""
    pooled, proj = clip_forward(pixel_values, w, geom, dtype, tok={"cls": 0, "last": geom.seq_len - 1}[pool], mutant=mutant)
    e = proj if proj is not None else pooled
    return e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
