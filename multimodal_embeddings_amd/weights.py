"""Deterministic synthetic ViT/16 weights: ViT-B/16 by default, any `ViTGeometry` (SURVEY.md §8d "Synthetic inputs").

The reference loads pretrained weights by NAME over the network
(deprecated_package/embedder.py:75-79), which is unavailable offline, so the
encoder of this build runs on seeded synthetic weights.  The generator is a
counter-based integer hash, so the very same tensors are produced in the build
container, on the GPU box and inside the golden-vector script without shipping
343 MB of floats:

    value(seed, tensor_id, i) = bf16_round( offset + std * z ),
    z = (sum of twelve 16-bit lanes of splitmix64 words - 393210) / 65536

(an Irwin-Hall approximation of N(0,1); every step is integer or a single
correctly-rounded IEEE operation, so no libm call can differ between hosts).
All values are bf16-representable: the reference itself runs its encoder with
``torch_dtype=torch.bfloat16`` (embedder.py:78), and this lets the fp32 oracle
and the bf16 MFMA path consume bit-identical parameters.

Tensor names follow the Hugging Face ViT checkpoint layout
(transformers/models/vit/modeling_vit.py; `ViTModel(add_pooling_layer=False)`)
so the same dict loads into that class with ``load_state_dict`` when the golden
vectors are generated.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

_MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)

# ---- what every tower's transformer block shares ------------------------------------------------------------------------
LAYER_FIELDS = ("ln1_g", "ln1_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "o_w", "o_b", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")  # _lib._Layer


def _block_names(ln1: str, ln2: str, q: str, k: str, v: str, o: str):
    """One spelling of a block: the tensor names (behind the layer's prefix) of LAYER_FIELDS, in that order."""
    return tuple(f"{m}.{p}" for m in (ln1, q, k, v, o, ln2, "mlp.fc1", "mlp.fc2") for p in ("weight", "bias"))


VIT_BLOCK = _block_names("layernorm_before", "layernorm_after", *(f"attention.{n}_proj" for n in "qkvo"))
CLIP_BLOCK = _block_names("layer_norm1", "layer_norm2", *(f"self_attn.{n}_proj" for n in ("q", "k", "v", "out")))  # CLIP and SigLIP, image and text
DINOV2_BLOCK = _block_names("norm1", "norm2", *(f"attention.attention.{n}" for n in ("query", "key", "value")), "attention.output.dense")


def block_tensor_specs(prefix: str, names, D: int, F: int):
    """(name, shape, kind) of one block's 16 tensors in LAYER_FIELDS order; `names`: a *_BLOCK spelling."""
    shapes = {"fc1_w": (F, D), "fc1_b": (F,), "fc2_w": (D, F)}
    specs = []
    for fld, name in zip(LAYER_FIELDS, names):
        kind = "gamma" if fld in ("ln1_g", "ln2_g") else "bias" if fld.endswith("_b") else "matrix"
        specs.append((prefix + name, shapes.get(fld, (D, D) if kind == "matrix" else (D,)), kind))
    return specs


def _layer_count(w: dict, key: str) -> int:
    """How many layers a weight dict holds, counted on `key` (a format over the layer index)."""
    layers = 0
    while key.format(layers) in w:
        layers += 1
    if layers == 0:
        raise ValueError(f"the weight dict holds no {key.format(0)!r}")
    return layers


def _seeded_weights(specs, seed: int, rule) -> dict[str, np.ndarray]:
    """The one generator: tensor `tid` of `specs` is bf16_round(rule(name, kind, z)), z = irwin_hall_normal(seed, tid, n)."""
    out: dict[str, np.ndarray] = {}
    for tid, (name, shape, kind) in enumerate(specs):
        out[name] = round_to_bf16(rule(name, kind, irwin_hall_normal(seed, tid, int(np.prod(shape))))).reshape(shape)
    return out


def _spread_rule(std: float, is_norm, unscaled=lambda name: False):
    """The rule of every tower but the plain ViT: LayerNorm weights 1 + 0.25 z and biases 0.1 z (`is_norm(name)` says which
    biases are a LayerNorm's), LayerScale's lambda1 1.025 + 0.325 z clipped to [0.05, 2], `unscaled(name)` tensors z itself,
    everything else std z."""
    def rule(name, kind, z):
        if kind == "gamma":
            return np.float32(1.0) + z * np.float32(0.25)
        if kind == "scale":
            return np.clip(np.float32(1.025) + z * np.float32(0.325), np.float32(0.05), np.float32(2.0))
        if kind == "bias" and is_norm(name):
            return z * np.float32(0.1)
        return z if unscaled(name) else z * np.float32(std)

    return rule


@dataclass(frozen=True)
class ViTGeometry:
    """A ViT/16 or ViT/32 @224 encoder (197 or 50 tokens); the defaults are ViT-B/16 (transformers ViTConfig defaults).  What the engine runs is
    `SUPPORTED_VIT` below (checked by `check_vit_geometry`, and again by the library when the weights are loaded)."""

    image_size: int = 224
    patch_size: int = 16
    num_channels: int = 3
    hidden_size: int = 768
    num_layers: int = 12
    num_heads: int = 12
    intermediate_size: int = 3072
    layer_norm_eps: float = 1e-12

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid * self.grid

    @property
    def seq_len(self) -> int:
        return self.num_patches + 1

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def patch_dim(self) -> int:
        return self.num_channels * self.patch_size * self.patch_size


VIT_B16 = ViTGeometry()
VIT_S16 = ViTGeometry(hidden_size=384, num_layers=12, num_heads=6, intermediate_size=1536)
VIT_L16 = ViTGeometry(hidden_size=1024, num_layers=24, num_heads=16, intermediate_size=4096)
VIT_B32 = ViTGeometry(patch_size=32)  # 7 x 7 patches of 32 x 32, 50 tokens (google/vit-base-patch32-224-in21k)

# the geometries the engine is built for (csrc/common.h, csrc/weight_load.hip validate_vit_weights)
SUPPORTED_VIT = {"image_size": (224,), "patch_size": (16, 32), "num_channels": (3,), "hidden_size": (384, 768, 1024), "head_dim": (64,),
                 "intermediate_size": "a multiple of 64 up to 8192", "num_layers": "1..64"}


def vit_geometry_problem(geom: ViTGeometry):
    """None when the engine runs `geom`, else (field, value found, supported values as text) of the first field outside
    the supported set."""
    for fld in ("image_size", "patch_size", "num_channels", "hidden_size"):
        if getattr(geom, fld) not in SUPPORTED_VIT[fld]:
            return fld, getattr(geom, fld), ", ".join(str(v) for v in SUPPORTED_VIT[fld])
    if geom.num_heads * 64 != geom.hidden_size:
        return "num_heads", geom.num_heads, f"{geom.hidden_size // 64} at hidden_size {geom.hidden_size} (heads of 64)"
    F = geom.intermediate_size
    if F < 64 or F % 64 or F > 8192:
        return "intermediate_size", F, SUPPORTED_VIT["intermediate_size"]
    if not 1 <= geom.num_layers <= 64:
        return "num_layers", geom.num_layers, SUPPORTED_VIT["num_layers"]
    return None


def vit_flops_per_crop(geom: ViTGeometry = VIT_B16) -> int:
    """FLOP of one crop's forward as DESIGN.md §4 counts them (2 per multiply-add; LayerNorm, softmax and GELU excluded):
    the patch embedding (196 x patch_dim x D) and, per layer, the four projections and the two MLP matrices on 197 tokens
    plus the two attention products.  DESIGN's figure for ViT-B/16, 35 126 083 584 (bench.py prices its headline with it),
    holds 4 (197^2 - 1) D per layer for the attention products -- 36 864 FLOP, one part in a million, below the plain
    4 x 197^2 x D; this function keeps DESIGN's count at every width so that the fractions of nominal it feeds compare
    with the recorded ones."""
    D, F, L, T = geom.hidden_size, geom.intermediate_size, geom.num_layers, geom.seq_len
    return 2 * geom.num_patches * geom.patch_dim * D + L * (2 * T * D * (4 * D + 2 * F) + 4 * (T * T - 1) * D)


def infer_vit_geometry(w: dict, eps: float = 1e-12) -> ViTGeometry:
    """The geometry of a canonical-name weight dict (vit_tensor_specs), read off its tensor shapes; heads of 64."""
    D = int(np.shape(w["embeddings.patch_embeddings.projection.weight"])[0])
    patch = int(np.shape(w["embeddings.patch_embeddings.projection.weight"])[-1])
    tokens = int(np.shape(w["embeddings.position_embeddings"])[-2])
    grid = int(round((tokens - 1) ** 0.5))
    layers = _layer_count(w, "layers.{}.mlp.fc1.weight")
    F = int(np.shape(w["layers.0.mlp.fc1.weight"])[0])
    return ViTGeometry(image_size=grid * patch, patch_size=patch, hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F,
                       layer_norm_eps=float(eps))


# ---- CLIP ViT/16 image towers ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class CLIPGeometry(ViTGeometry):
    """A CLIP image tower at the engine's ViT/16 or ViT/32 @224 geometry (transformers CLIPVisionConfig): the ViT fields, with
    layer_norm_eps 1e-5, plus the width of the shared image / text space (`projection_dim`; None: no visual_projection,
    the embedding is the post_layernorm row) and the MLP activation ("quick_gelu": OpenAI weights, "gelu": LAION
    conversions).  The defaults are clip-vit-base-patch16."""

    layer_norm_eps: float = 1e-5
    projection_dim: int | None = 512
    hidden_act: str = "quick_gelu"

    @property
    def embed_dim(self) -> int:
        return self.projection_dim or self.hidden_size


CLIP_B16 = CLIPGeometry()
CLIP_B32 = CLIPGeometry(patch_size=32)  # clip-vit-base-patch32: 768 x 12, MLP 3072, projection 512, quick_gelu, 50 tokens
CLIP_ACTS = ("gelu", "quick_gelu")  # include/mme.h mme_clip_weights.act: the index


def clip_geometry_problem(geom: CLIPGeometry):
    """As `vit_geometry_problem`, with the two CLIP fields: None, or (field, value found, supported values as text)."""
    bad = vit_geometry_problem(geom)
    if bad:
        return bad
    if geom.hidden_act not in CLIP_ACTS:
        return "hidden_act", geom.hidden_act, ", ".join(CLIP_ACTS)
    P = geom.projection_dim
    if P is not None and (isinstance(P, bool) or not isinstance(P, int) or P < 64 or P % 64 or P > 1024):
        return "projection_dim", P, "absent, or a multiple of 64 up to 1024"
    return None


def clip_tensor_specs(geom: CLIPGeometry = CLIP_B16):
    """(name, shape, kind) in a fixed order, Hugging Face `CLIPVisionModelWithProjection` state-dict names
    (transformers models/clip/modeling_clip.py); kind in {matrix, bias, gamma}.  Without `projection_dim` the list ends
    at post_layernorm (`CLIPVisionModel`)."""
    D, F, P = geom.hidden_size, geom.intermediate_size, geom.patch_size
    v = "vision_model."
    specs = [
        (v + "embeddings.class_embedding", (D,), "matrix"),
        (v + "embeddings.patch_embedding.weight", (D, geom.num_channels, P, P), "matrix"),
        (v + "embeddings.position_embedding.weight", (geom.seq_len, D), "matrix"),
        (v + "pre_layrnorm.weight", (D,), "gamma"),
        (v + "pre_layrnorm.bias", (D,), "bias"),
    ]
    for i in range(geom.num_layers):
        specs += block_tensor_specs(f"{v}encoder.layers.{i}.", CLIP_BLOCK, D, F)
    specs += [(v + "post_layernorm.weight", (D,), "gamma"), (v + "post_layernorm.bias", (D,), "bias")]
    if geom.projection_dim:
        specs.append(("visual_projection.weight", (geom.projection_dim, D), "matrix"))
    return specs


def make_clip_weights(seed: int = 1, geom: CLIPGeometry = CLIP_B16, std: float = 0.02) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of a CLIP image tower, f32 arrays holding bf16-representable values; the generator of
    `make_vit_weights` on `clip_tensor_specs`.  LayerNorm weights are 1 + 0.25 z and biases 0.1 z (z ~ N(0, 1)): far enough
    from 1 and 0 that a dropped LayerNorm, or two LayerNorms exchanged, moves the embedding by much more than the bf16
    path's error.  Matrices N(0, std), the other biases N(0, std)."""
    return _seeded_weights(clip_tensor_specs(geom), seed, _spread_rule(std, lambda name: "layer_norm" in name or "layrnorm" in name or "layernorm" in name))


def clip_flops_per_crop(geom: CLIPGeometry = CLIP_B16) -> int:
    """`vit_flops_per_crop` plus the projection of the pooled row (2 D P); pre_layrnorm, like every LayerNorm, is not counted."""
    return vit_flops_per_crop(geom) + 2 * geom.hidden_size * (geom.projection_dim or 0)


def infer_clip_geometry(w: dict, eps: float = 1e-5, hidden_act: str = "quick_gelu") -> CLIPGeometry:
    """The geometry of a `clip_tensor_specs` weight dict, read off its tensor shapes; heads of 64.  The activation is not in
    the tensors: `hidden_act` names it."""
    pw = np.shape(w["vision_model.embeddings.patch_embedding.weight"])
    D, patch = int(pw[0]), int(pw[-1])
    tokens = int(np.shape(w["vision_model.embeddings.position_embedding.weight"])[0])
    grid = int(round((tokens - 1) ** 0.5))
    layers = _layer_count(w, "vision_model.encoder.layers.{}.mlp.fc1.weight")
    F = int(np.shape(w["vision_model.encoder.layers.0.mlp.fc1.weight"])[0])
    P = int(np.shape(w["visual_projection.weight"])[0]) if "visual_projection.weight" in w else None
    return CLIPGeometry(image_size=grid * patch, patch_size=patch, hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F,
                        layer_norm_eps=float(eps), projection_dim=P, hidden_act=hidden_act)


# ---- SigLIP ViT/16 image towers ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SiglipGeometry(ViTGeometry):
    """A SigLIP image tower at the engine's ViT/16 @224 geometry (transformers SiglipVisionConfig): the ViT fields with
    layer_norm_eps 1e-6, no class token (196 tokens), `gelu_pytorch_tanh` in every MLP and the attention-pooling head
    (`vision_use_head`).  The embedding is the head's output, `hidden_size` wide.  The defaults are siglip-base-patch16-224."""

    layer_norm_eps: float = 1e-6
    hidden_act: str = "gelu_pytorch_tanh"
    vision_use_head: bool = True

    @property
    def seq_len(self) -> int:
        return self.num_patches

    @property
    def embed_dim(self) -> int:
        return self.hidden_size


SIGLIP_B16 = SiglipGeometry()
SUPPORTED_SIGLIP = {"patch_size": (16,), "hidden_act": ("gelu_pytorch_tanh",), "vision_use_head": (True,)}


def siglip_geometry_problem(geom: SiglipGeometry):
    """As `vit_geometry_problem` with patch 16 only and the two SigLIP fields: None, or (field, value found, supported values as text)."""
    if geom.patch_size not in SUPPORTED_SIGLIP["patch_size"]:
        return "patch_size", geom.patch_size, "16"
    bad = vit_geometry_problem(geom)
    if bad:
        return bad
    if geom.hidden_act not in SUPPORTED_SIGLIP["hidden_act"]:
        return "hidden_act", geom.hidden_act, "gelu_pytorch_tanh"
    if geom.vision_use_head is not True:
        return "vision_use_head", geom.vision_use_head, "True (the attention-pooling head)"
    return None


def siglip_tensor_specs(geom: SiglipGeometry = SIGLIP_B16):
    """(name, shape, kind) in a fixed order, the state-dict names of a `SiglipVisionModel` inside a `SiglipModel`
    (transformers models/siglip/modeling_siglip.py; prefix "vision_model."); kind in {matrix, bias, gamma}."""
    D, F, P = geom.hidden_size, geom.intermediate_size, geom.patch_size
    v = "vision_model."
    specs = [
        (v + "embeddings.patch_embedding.weight", (D, geom.num_channels, P, P), "matrix"),
        (v + "embeddings.patch_embedding.bias", (D,), "bias"),
        (v + "embeddings.position_embedding.weight", (geom.seq_len, D), "matrix"),
    ]
    for i in range(geom.num_layers):
        specs += block_tensor_specs(f"{v}encoder.layers.{i}.", CLIP_BLOCK, D, F)
    h = v + "head."
    specs += [
        (v + "post_layernorm.weight", (D,), "gamma"),
        (v + "post_layernorm.bias", (D,), "bias"),
        (h + "probe", (1, 1, D), "matrix"),
        (h + "attention.in_proj_weight", (3 * D, D), "matrix"),
        (h + "attention.in_proj_bias", (3 * D,), "bias"),
        (h + "attention.out_proj.weight", (D, D), "matrix"),
        (h + "attention.out_proj.bias", (D,), "bias"),
        (h + "layernorm.weight", (D,), "gamma"),
        (h + "layernorm.bias", (D,), "bias"),
        (h + "mlp.fc1.weight", (F, D), "matrix"),
        (h + "mlp.fc1.bias", (F,), "bias"),
        (h + "mlp.fc2.weight", (D, F), "matrix"),
        (h + "mlp.fc2.bias", (D,), "bias"),
    ]
    return specs


def make_siglip_weights(seed: int = 4, geom: SiglipGeometry = SIGLIP_B16, std: float = 0.02) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of a SigLIP image tower, f32 arrays holding bf16-representable values: the generator and the
    LayerNorm spread of `make_clip_weights` on `siglip_tensor_specs`.  The probe is N(0, 1) as transformers initialises it,
    so that the head's scores are spread over the keys instead of near-uniform."""
    return _seeded_weights(siglip_tensor_specs(geom), seed, _spread_rule(std, lambda name: "layer_norm" in name or "layernorm" in name,
                                                                         unscaled=lambda name: name.endswith("head.probe")))


def siglip_flops_per_crop(geom: SiglipGeometry = SIGLIP_B16) -> int:
    """`vit_flops_per_crop` at 196 tokens plus the head: K | V over the 196 tokens (4 T D^2), the pooled attention (4 T D),
    out_proj (2 D^2) and the head's MLP (4 D F)."""
    D, F, T = geom.hidden_size, geom.intermediate_size, geom.seq_len
    return vit_flops_per_crop(geom) + 4 * T * D * D + 4 * T * D + 2 * D * D + 4 * D * F


def infer_siglip_geometry(w: dict, eps: float = 1e-6) -> SiglipGeometry:
    """The geometry of a `siglip_tensor_specs` weight dict, read off its tensor shapes; heads of 64."""
    pw = np.shape(w["vision_model.embeddings.patch_embedding.weight"])
    D, patch = int(pw[0]), int(pw[-1])
    tokens = int(np.shape(w["vision_model.embeddings.position_embedding.weight"])[0])
    grid = int(round(tokens ** 0.5))
    layers = _layer_count(w, "vision_model.encoder.layers.{}.mlp.fc1.weight")
    F = int(np.shape(w["vision_model.encoder.layers.0.mlp.fc1.weight"])[0])
    return SiglipGeometry(image_size=grid * patch, patch_size=patch, hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F,
                          layer_norm_eps=float(eps))


# ---- DINOv2 ViT/14 image towers ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Dinov2Geometry(ViTGeometry):
    """A DINOv2 image tower at the engine's third geometry (transformers Dinov2Config): patch 14 at 224 pixels, 16 x 16 patches
    and a class token (257 tokens), heads of 64, layer_norm_eps 1e-6, erf-GELU, an MLP of `mlp_ratio` x hidden, LayerScale
    behind the attention and the MLP of every block.  `position_grid` is the side of the checkpoint's patch position grid: 16
    (a 257-row table, taken as it is) or 37 (`image_size` 518 in config.json, 1370 rows: dinov2-small / -base / -large), which
    the loader interpolates to 16 x 16 once, on the host.  The embedding is `pooler_output`, `hidden_size` wide.  The defaults
    are dinov2-base."""

    patch_size: int = 14
    layer_norm_eps: float = 1e-6
    hidden_act: str = "gelu"
    use_swiglu_ffn: bool = False
    num_register_tokens: int = 0
    position_grid: int = 16

    @property
    def patch_dim_padded(self) -> int:
        return (self.patch_dim + 63) // 64 * 64  # 588 -> 640: K of the patch-embed GEMM

    @property
    def embed_dim(self) -> int:
        return self.hidden_size

    @property
    def position_rows(self) -> int:
        return 1 + self.position_grid * self.position_grid


DINOV2_S14 = Dinov2Geometry(hidden_size=384, num_layers=12, num_heads=6, intermediate_size=1536)
DINOV2_B14 = Dinov2Geometry()
DINOV2_L14 = Dinov2Geometry(hidden_size=1024, num_layers=24, num_heads=16, intermediate_size=4096)
SUPPORTED_DINOV2 = {"patch_size": (14,), "hidden_act": ("gelu",), "use_swiglu_ffn": (False,), "num_register_tokens": (0,)}


def dinov2_geometry_problem(geom: Dinov2Geometry):
    """As `vit_geometry_problem` with patch 14 only and the DINOv2 fields: None, or (field, value found, supported values as text)."""
    if geom.use_swiglu_ffn is not False:
        return "use_swiglu_ffn", geom.use_swiglu_ffn, "False (the SwiGLU MLP of dinov2-giant is not run)"
    if geom.num_register_tokens != 0:
        return "num_register_tokens", geom.num_register_tokens, "0 (Dinov2WithRegisters is not run)"
    if geom.patch_size not in SUPPORTED_DINOV2["patch_size"]:
        return "patch_size", geom.patch_size, "14"
    for fld in ("image_size", "num_channels", "hidden_size"):
        if getattr(geom, fld) not in SUPPORTED_VIT[fld]:
            return fld, getattr(geom, fld), ", ".join(str(v) for v in SUPPORTED_VIT[fld])
    if geom.num_heads * 64 != geom.hidden_size:
        return "num_heads", geom.num_heads, f"{geom.hidden_size // 64} at hidden_size {geom.hidden_size} (heads of 64)"
    F = geom.intermediate_size
    if F < 64 or F % 64 or F > 8192:
        return "intermediate_size", F, SUPPORTED_VIT["intermediate_size"]
    if not 1 <= geom.num_layers <= 64:
        return "num_layers", geom.num_layers, SUPPORTED_VIT["num_layers"]
    if geom.hidden_act not in SUPPORTED_DINOV2["hidden_act"]:
        return "hidden_act", geom.hidden_act, "gelu"
    if geom.position_grid < 1:
        return "position_grid", geom.position_grid, "a positive grid side"
    return None


def dinov2_tensor_specs(geom: Dinov2Geometry = DINOV2_B14):
    """(name, shape, kind) in a fixed order, the state-dict names of transformers' `Dinov2Model`
    (models/dinov2/modeling_dinov2.py); kind in {matrix, bias, gamma, scale}.  `embeddings.mask_token` is not listed: the
    forward without masked positions never reads it."""
    D, F, P = geom.hidden_size, geom.intermediate_size, geom.patch_size
    specs = [
        ("embeddings.cls_token", (1, 1, D), "matrix"),
        ("embeddings.position_embeddings", (1, geom.position_rows, D), "matrix"),
        ("embeddings.patch_embeddings.projection.weight", (D, geom.num_channels, P, P), "matrix"),
        ("embeddings.patch_embeddings.projection.bias", (D,), "bias"),
    ]
    for i in range(geom.num_layers):
        p = f"encoder.layer.{i}."
        block = block_tensor_specs(p, DINOV2_BLOCK, D, F)  # LayerScale sits behind the attention's output and behind the MLP
        specs += block[:10] + [(p + "layer_scale1.lambda1", (D,), "scale")] + block[10:] + [(p + "layer_scale2.lambda1", (D,), "scale")]
    specs += [("layernorm.weight", (D,), "gamma"), ("layernorm.bias", (D,), "bias")]
    return specs


def make_dinov2_weights(seed: int = 6, geom: Dinov2Geometry = DINOV2_B14, std: float = 0.02, pos_grid: int | None = None) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of a DINOv2 tower, f32 arrays holding bf16-representable values: the generator and the
    LayerNorm spread of `make_clip_weights` on `dinov2_tensor_specs`.  LayerScale's lambda1 is drawn from about [0.05, 2]
    (1.025 + 0.325 z clipped), far from the constant 1 a dropped or exchanged scale would be, so that the fold at load time
    is exercised.  `pos_grid` (16 or 37) overrides the geometry's position grid: 37 gives the 1370-row table real
    checkpoints carry."""
    import dataclasses

    if pos_grid is not None:
        geom = dataclasses.replace(geom, position_grid=int(pos_grid))
    return _seeded_weights(dinov2_tensor_specs(geom), seed, _spread_rule(std, lambda name: ".norm" in name or "layernorm" in name))


def dinov2_flops_per_crop(geom: Dinov2Geometry = DINOV2_B14) -> int:
    """`vit_flops_per_crop`'s count at 257 tokens, the patch embedding at its real K of 588 (the padded columns are zeros)."""
    D, F, L, T = geom.hidden_size, geom.intermediate_size, geom.num_layers, geom.seq_len
    return 2 * geom.num_patches * geom.patch_dim * D + L * (2 * T * D * (4 * D + 2 * F) + 4 * T * T * D)


def infer_dinov2_geometry(w: dict, eps: float = 1e-6) -> Dinov2Geometry:
    """The geometry of a `dinov2_tensor_specs` weight dict, read off its tensor shapes; heads of 64, 224 pixels.  A position
    table whose patch part is no square grid raises, naming the tensor."""
    pw = np.shape(w["embeddings.patch_embeddings.projection.weight"])
    D, patch = int(pw[0]), int(pw[-1])
    rows = int(np.shape(w["embeddings.position_embeddings"])[-2])
    grid = int(round((rows - 1) ** 0.5))
    if rows < 2 or grid * grid != rows - 1:
        raise ValueError(f"tensor 'embeddings.position_embeddings' has {rows} rows: the patch part ({rows - 1} rows) is no square grid")
    layers = _layer_count(w, "encoder.layer.{}.mlp.fc1.weight")
    F = int(np.shape(w["encoder.layer.0.mlp.fc1.weight"])[0])
    return Dinov2Geometry(image_size=224, patch_size=patch, hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F,
                          layer_norm_eps=float(eps), position_grid=grid)


# ---- CLIP text towers -------------------------------------------------------------------------------------------------
TEXT_TOKENS = 77  # CLIPTextConfig.max_position_embeddings; fixed at compile time (csrc/common.h TXT_T)


@dataclass(frozen=True)
class CLIPTextGeometry:
    """A CLIP text tower (transformers CLIPTextConfig) at what the engine runs: 77 positions, heads of 64.  The defaults are
    clip-vit-base-patch16's text tower.  `projection_dim` None: no text_projection (`CLIPTextModel`), the embedding is the
    final_layer_norm row at the EOS position.  `eos_token_id` 2 selects transformers' legacy pooling rule (the position of
    the sequence's largest id)."""

    hidden_size: int = 512
    num_layers: int = 12
    num_heads: int = 8
    intermediate_size: int = 2048
    vocab_size: int = 49408
    max_position_embeddings: int = TEXT_TOKENS
    eos_token_id: int = 49407
    projection_dim: int | None = 512
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5

    @property
    def embed_dim(self) -> int:
        return self.projection_dim or self.hidden_size


CLIP_TEXT_B = CLIPTextGeometry()
SUPPORTED_CLIP_TEXT = {"hidden_size": (512, 768, 1024), "max_position_embeddings": (TEXT_TOKENS,), "intermediate_size": "a multiple of 64 up to 8192",
                       "num_layers": "1..64", "vocab_size": "3..65536", "projection_dim": "absent, or a multiple of 64 up to 1024"}


def clip_text_geometry_problem(geom: CLIPTextGeometry):
    """None when the engine runs `geom`, else (field, value found, supported values as text) of the first field outside the
    supported set (csrc/capi_text.hip validate_text_weights)."""
    for fld in ("hidden_size", "max_position_embeddings"):
        if getattr(geom, fld) not in SUPPORTED_CLIP_TEXT[fld]:
            return fld, getattr(geom, fld), ", ".join(str(v) for v in SUPPORTED_CLIP_TEXT[fld])
    if geom.num_heads * 64 != geom.hidden_size:
        return "num_heads", geom.num_heads, f"{geom.hidden_size // 64} at hidden_size {geom.hidden_size} (heads of 64)"
    F = geom.intermediate_size
    if F < 64 or F % 64 or F > 8192:
        return "intermediate_size", F, SUPPORTED_CLIP_TEXT["intermediate_size"]
    if not 1 <= geom.num_layers <= 64:
        return "num_layers", geom.num_layers, SUPPORTED_CLIP_TEXT["num_layers"]
    if not 3 <= geom.vocab_size <= 65536:
        return "vocab_size", geom.vocab_size, SUPPORTED_CLIP_TEXT["vocab_size"]
    if geom.hidden_act not in CLIP_ACTS:
        return "hidden_act", geom.hidden_act, ", ".join(CLIP_ACTS)
    P = geom.projection_dim
    if P is not None and (isinstance(P, bool) or not isinstance(P, int) or P < 64 or P % 64 or P > 1024):
        return "projection_dim", P, SUPPORTED_CLIP_TEXT["projection_dim"]
    if isinstance(geom.eos_token_id, bool) or not isinstance(geom.eos_token_id, int) or not 0 <= geom.eos_token_id < geom.vocab_size:
        return "eos_token_id", geom.eos_token_id, f"0..{geom.vocab_size - 1} (vocab_size - 1)"
    return None


def clip_text_tensor_specs(geom: CLIPTextGeometry = CLIP_TEXT_B):
    """(name, shape, kind) in a fixed order, the state-dict names of Hugging Face `CLIPTextModelWithProjection`
    (transformers models/clip/modeling_clip.py); kind in {matrix, bias, gamma}.  Without `projection_dim` the list ends at
    final_layer_norm (`CLIPTextModel`)."""
    D, F = geom.hidden_size, geom.intermediate_size
    t = "text_model."
    specs = [
        (t + "embeddings.token_embedding.weight", (geom.vocab_size, D), "matrix"),
        (t + "embeddings.position_embedding.weight", (geom.max_position_embeddings, D), "matrix"),
    ]
    for i in range(geom.num_layers):
        specs += block_tensor_specs(f"{t}encoder.layers.{i}.", CLIP_BLOCK, D, F)
    specs += [(t + "final_layer_norm.weight", (D,), "gamma"), (t + "final_layer_norm.bias", (D,), "bias")]
    if geom.projection_dim:
        specs.append(("text_projection.weight", (geom.projection_dim, D), "matrix"))
    return specs


def make_clip_text_weights(seed: int = 3, geom: CLIPTextGeometry = CLIP_TEXT_B, std: float = 0.02) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of a CLIP text tower, f32 arrays holding bf16-representable values: the generator and the
    LayerNorm spread (1 + 0.25 z, 0.1 z) of `make_clip_weights` on `clip_text_tensor_specs`."""
    return _seeded_weights(clip_text_tensor_specs(geom), seed, _spread_rule(std, lambda name: "layer_norm" in name))


def infer_clip_text_geometry(w: dict, eps: float = 1e-5, hidden_act: str = "quick_gelu", eos_token_id: int | None = None) -> CLIPTextGeometry:
    """The geometry of a `clip_text_tensor_specs` weight dict, read off its tensor shapes; heads of 64.  What is not in the
    tensors is named by the caller: the activation, eps and `eos_token_id` (default: the last id of the table, where CLIP's
    vocabulary keeps <|endoftext|>)."""
    V, D = (int(v) for v in np.shape(w["text_model.embeddings.token_embedding.weight"]))
    T = int(np.shape(w["text_model.embeddings.position_embedding.weight"])[0])
    layers = _layer_count(w, "text_model.encoder.layers.{}.mlp.fc1.weight")
    F = int(np.shape(w["text_model.encoder.layers.0.mlp.fc1.weight"])[0])
    P = int(np.shape(w["text_projection.weight"])[0]) if "text_projection.weight" in w else None
    return CLIPTextGeometry(hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F, vocab_size=V, max_position_embeddings=T,
                            eos_token_id=V - 1 if eos_token_id is None else int(eos_token_id), projection_dim=P, hidden_act=hidden_act,
                            layer_norm_eps=float(eps))


def clip_text_flops_per_sequence(geom: CLIPTextGeometry = CLIP_TEXT_B) -> int:
    """FLOP of one sequence's forward counted as `vit_flops_per_crop` counts (2 per multiply-add; LayerNorm, softmax and the
    activation excluded): per layer the four projections and the two MLP matrices on 77 tokens plus the two attention
    products over the T (T + 1) / 2 unmasked (query, key) pairs, then the projection of the pooled row.  All 77 rows are
    counted: the pass computes the rows behind the EOS too."""
    D, F, L, T = geom.hidden_size, geom.intermediate_size, geom.num_layers, geom.max_position_embeddings
    return L * (2 * T * D * (4 * D + 2 * F) + 4 * (T * (T + 1) // 2) * D) + 2 * D * (geom.projection_dim or 0)


# ---- SigLIP text towers -----------------------------------------------------------------------------------------------
SIGLIP_TEXT_TOKENS = 64  # SiglipTextConfig.max_position_embeddings (csrc/common.h TXT_T64)
SIGLIP_TEXT_ACT = "gelu_pytorch_tanh"


@dataclass(frozen=True)
class SiglipTextGeometry:
    """A SigLIP text tower (transformers SiglipTextConfig) at what the engine runs: 64 positions, heads of 64, no attention mask,
    the row at position 63 pooled, a head with bias onto `projection_size`.  The defaults are siglip-base-patch16-224's text
    tower.  `pad_token_id` is what short sequences are right-padded with (SigLIP's tokenizer: 1; the padding is attended)."""

    hidden_size: int = 768
    num_layers: int = 12
    num_heads: int = 12
    intermediate_size: int = 3072
    vocab_size: int = 32000
    max_position_embeddings: int = SIGLIP_TEXT_TOKENS
    pad_token_id: int = 1
    projection_size: int = 768
    hidden_act: str = SIGLIP_TEXT_ACT
    layer_norm_eps: float = 1e-6

    @property
    def embed_dim(self) -> int:
        return self.projection_size


SIGLIP_TEXT_B = SiglipTextGeometry()
SUPPORTED_SIGLIP_TEXT = {"hidden_size": (512, 768, 1024), "max_position_embeddings": (SIGLIP_TEXT_TOKENS,),
                         "intermediate_size": "a multiple of 64 up to 8192", "num_layers": "1..64", "vocab_size": "3..262144",
                         "projection_size": "a multiple of 64 up to 1024", "hidden_act": (SIGLIP_TEXT_ACT,)}


def siglip_text_geometry_problem(geom: SiglipTextGeometry):
    """None when the engine runs `geom`, else (field, value found, supported values as text) of the first field outside the
    supported set (csrc/capi_text.hip validate_siglip_text_weights).  so400m (hidden 1152, heads of 72) stops at hidden_size."""
    for fld in ("hidden_size", "max_position_embeddings"):
        if getattr(geom, fld) not in SUPPORTED_SIGLIP_TEXT[fld]:
            return fld, getattr(geom, fld), ", ".join(str(v) for v in SUPPORTED_SIGLIP_TEXT[fld])
    if geom.num_heads * 64 != geom.hidden_size:
        return "num_heads", geom.num_heads, f"{geom.hidden_size // 64} at hidden_size {geom.hidden_size} (heads of 64)"
    F = geom.intermediate_size
    if F < 64 or F % 64 or F > 8192:
        return "intermediate_size", F, SUPPORTED_SIGLIP_TEXT["intermediate_size"]
    if not 1 <= geom.num_layers <= 64:
        return "num_layers", geom.num_layers, SUPPORTED_SIGLIP_TEXT["num_layers"]
    if not 3 <= geom.vocab_size <= 262144:
        return "vocab_size", geom.vocab_size, SUPPORTED_SIGLIP_TEXT["vocab_size"]
    if geom.hidden_act not in SUPPORTED_SIGLIP_TEXT["hidden_act"]:
        return "hidden_act", geom.hidden_act, SIGLIP_TEXT_ACT
    P = geom.projection_size
    if isinstance(P, bool) or not isinstance(P, int) or P < 64 or P % 64 or P > 1024:
        return "projection_size", P, SUPPORTED_SIGLIP_TEXT["projection_size"]
    if isinstance(geom.pad_token_id, bool) or not isinstance(geom.pad_token_id, int) or not 0 <= geom.pad_token_id < geom.vocab_size:
        return "pad_token_id", geom.pad_token_id, f"0..{geom.vocab_size - 1} (vocab_size - 1)"
    return None


def siglip_text_tensor_specs(geom: SiglipTextGeometry = SIGLIP_TEXT_B):
    """(name, shape, kind) in a fixed order, the state-dict names of the text half of a Hugging Face `SiglipModel`
    (transformers models/siglip/modeling_siglip.py; prefix "text_model."); kind in {matrix, bias, gamma}.  The two scalars
    `logit_scale` / `logit_bias` of a whole model are not in the list: a weight dict may carry them beside these tensors."""
    D, F = geom.hidden_size, geom.intermediate_size
    t = "text_model."
    specs = [
        (t + "embeddings.token_embedding.weight", (geom.vocab_size, D), "matrix"),
        (t + "embeddings.position_embedding.weight", (geom.max_position_embeddings, D), "matrix"),
    ]
    for i in range(geom.num_layers):
        specs += block_tensor_specs(f"{t}encoder.layers.{i}.", CLIP_BLOCK, D, F)
    specs += [(t + "final_layer_norm.weight", (D,), "gamma"), (t + "final_layer_norm.bias", (D,), "bias"),
              (t + "head.weight", (geom.projection_size, D), "matrix"), (t + "head.bias", (geom.projection_size,), "bias")]
    return specs


SIGLIP_LOGIT_KEYS = ("logit_scale", "logit_bias")


def make_siglip_text_weights(seed: int = 5, geom: SiglipTextGeometry = SIGLIP_TEXT_B, std: float = 0.02, logits=(np.log(10.0), -10.0)) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of a SigLIP text tower, f32 arrays holding bf16-representable values: the generator and the
    LayerNorm spread (1 + 0.25 z, 0.1 z) of `make_clip_weights` on `siglip_text_tensor_specs`.  `logits`: (logit_scale,
    logit_bias) as f32 arrays of shape (1,) beside the tensors (SiglipModel initialises them to log 10 and -10); None: left out."""
    out = _seeded_weights(siglip_text_tensor_specs(geom), seed, _spread_rule(std, lambda name: "layer_norm" in name))
    if logits is not None:
        out["logit_scale"] = round_to_bf16(np.array([logits[0]], dtype=np.float32))
        out["logit_bias"] = round_to_bf16(np.array([logits[1]], dtype=np.float32))
    return out


def infer_siglip_text_geometry(w: dict, eps: float = 1e-6, pad_token_id: int = 1) -> SiglipTextGeometry:
    """The geometry of a `siglip_text_tensor_specs` weight dict, read off its tensor shapes; heads of 64."""
    V, D = (int(v) for v in np.shape(w["text_model.embeddings.token_embedding.weight"]))
    T = int(np.shape(w["text_model.embeddings.position_embedding.weight"])[0])
    layers = _layer_count(w, "text_model.encoder.layers.{}.mlp.fc1.weight")
    F = int(np.shape(w["text_model.encoder.layers.0.mlp.fc1.weight"])[0])
    P = int(np.shape(w["text_model.head.weight"])[0])
    return SiglipTextGeometry(hidden_size=D, num_layers=layers, num_heads=D // 64, intermediate_size=F, vocab_size=V, max_position_embeddings=T,
                              pad_token_id=int(pad_token_id), projection_size=P, layer_norm_eps=float(eps))


def siglip_text_flops_per_sequence(geom: SiglipTextGeometry = SIGLIP_TEXT_B) -> int:
    """`clip_text_flops_per_sequence` without a mask: all T * T (query, key) pairs, 64 rows, then the head on the pooled row."""
    D, F, L, T = geom.hidden_size, geom.intermediate_size, geom.num_layers, geom.max_position_embeddings
    return L * (2 * T * D * (4 * D + 2 * F) + 4 * T * T * D) + 2 * D * geom.projection_size


def siglip_token_ids(n: int, vocab: int, pad: int = 1, seed: int = 0, lengths=None) -> np.ndarray:
    """int32 [n, 64] right-padded sequences as SigLIP's tokenizer writes them under padding="max_length": sequence i holds
    lengths[i] hashed ids, none of them `pad`, then `pad` in every position behind.  `lengths` defaults to hashed values in 1..64."""
    T = SIGLIP_TEXT_TOKENS
    if lengths is None:
        lengths = 1 + (counter_u64(seed, 0x7200, n) % np.uint64(T)).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.shape[0] != n or (n and (lengths.min() < 0 or lengths.max() > T)):
        raise ValueError(f"lengths must hold {n} values in 0..{T}")
    out = np.full((n, T), pad, dtype=np.int32)
    for i in range(n):
        body = (counter_u64(seed, 0x7201, T, i) % np.uint64(vocab - 1)).astype(np.int64)
        body += body >= pad  # 0..vocab-1 without pad
        out[i, : lengths[i]] = body[: lengths[i]]
    return out


def synthetic_token_ids(n: int, vocab: int, eos: int, seed: int = 0, lengths=None) -> np.ndarray:
    """int32 [n, 77] BOS-free, right-padded sequences: sequence i holds lengths[i] - 1 hashed ids, none of them `eos`, then
    `eos` at position lengths[i] - 1 and in every position behind it (the padding CLIP's tokenizer writes).  `lengths`
    defaults to hashed values in 2..77."""
    if lengths is None:
        lengths = 2 + (counter_u64(seed, 0x7100, n) % np.uint64(TEXT_TOKENS - 1)).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.shape[0] != n or lengths.min() < 1 or lengths.max() > TEXT_TOKENS:
        raise ValueError(f"lengths must hold {n} values in 1..{TEXT_TOKENS}")
    out = np.full((n, TEXT_TOKENS), eos, dtype=np.int32)
    for i in range(n):
        body = (counter_u64(seed, 0x7101, TEXT_TOKENS, i) % np.uint64(vocab - 1)).astype(np.int64)
        body += body >= eos  # 0..vocab-1 without eos
        out[i, : lengths[i] - 1] = body[: lengths[i] - 1]
    return out


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _MASK64
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK64
        z = z ^ (z >> np.uint64(31))
    return z


def counter_u64(seed: int, stream: int, n: int, word: int = 0) -> np.ndarray:
    """n hashed 64-bit words for counters (seed, stream, i, word)."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = (
            np.uint64(seed & 0xFFFF) * np.uint64(1 << 48)
            + np.uint64(stream & 0xFFFF) * np.uint64(1 << 32)
        )
        key = _splitmix64(np.uint64(base) + np.uint64(word) * np.uint64(0xD1B54A32D192ED03))
        return _splitmix64(key ^ (i * np.uint64(0x2545F4914F6CDD1D)))


def irwin_hall_normal(seed: int, stream: int, n: int) -> np.ndarray:
    """Approximate N(0,1) float32 samples with exact integer provenance."""
    total = np.zeros(n, dtype=np.int64)
    for word in range(3):
        w = counter_u64(seed, stream, n, word)
        for lane in range(4):
            total += ((w >> np.uint64(16 * lane)) & np.uint64(0xFFFF)).astype(np.int64)
    # mean of twelve U{0..65535} is 12*32767.5 = 393210; var = 12*(65536^2-1)/12
    return ((total - 393210).astype(np.float32)) * np.float32(1.0 / 65536.0)


def round_to_bf16(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even f32 -> bf16, returned as f32 (finite inputs only)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    with np.errstate(over="ignore"):
        r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """bf16 bit pattern (uint16) of finite f32 values, round-to-nearest-even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    with np.errstate(over="ignore"):
        r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return r.astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def vit_tensor_specs(geom: ViTGeometry = VIT_B16):
    """(name, shape, kind) in a fixed order; kind in {matrix, bias, gamma}."""
    D, F, P = geom.hidden_size, geom.intermediate_size, geom.patch_size
    specs = [
        ("embeddings.cls_token", (1, 1, D), "matrix"),
        ("embeddings.position_embeddings", (1, geom.seq_len, D), "matrix"),
        ("embeddings.patch_embeddings.projection.weight", (D, geom.num_channels, P, P), "matrix"),
        ("embeddings.patch_embeddings.projection.bias", (D,), "bias"),
    ]
    for i in range(geom.num_layers):
        specs += block_tensor_specs(f"layers.{i}.", VIT_BLOCK, D, F)
    specs += [("layernorm.weight", (D,), "gamma"), ("layernorm.bias", (D,), "bias")]
    return specs


def make_vit_weights(
    seed: int = 1,
    geom: ViTGeometry = VIT_B16,
    std: float = 0.02,
    trained_like: bool = True,
) -> dict[str, np.ndarray]:
    """Seeded synthetic weights, f32 arrays holding bf16-representable values.

    ``trained_like=False`` reproduces the Hugging Face initialiser exactly as
    SURVEY.md §8d words it (biases 0, LayerNorm gamma 1 / beta 0).  The default
    perturbs biases and LayerNorm parameters as well, so that every bias-add and
    affine path of the kernels carries non-trivial data in the parity tests; the
    arithmetic cost is identical.
    """
    def rule(name, kind, z):
        if kind == "matrix" or trained_like:
            z = z * np.float32(std)
            return z + np.float32(1.0) if kind == "gamma" else z
        return np.full(z.shape, 1.0 if kind == "gamma" else 0.0, dtype=np.float32)

    return _seeded_weights(vit_tensor_specs(geom), seed, rule)


def synthetic_crops(n: int, seed: int = 0, size: int = 224, start: int = 0) -> np.ndarray:
    """uint8[n, size, size, 3] i.i.d. uniform 0..255 (SURVEY.md §8d, C2/C4 inputs).

    ``start`` offsets the crop index so that a rank can generate only its shard.
    """
    per = size * size * 3
    assert per % 8 == 0
    out = np.empty((n, per), dtype=np.uint8)
    words = per // 8
    for k in range(n):
        w = counter_u64(seed, 0x7000 + ((start + k) >> 16), words, (start + k) & 0xFFFF)
        out[k] = w.view(np.uint8)
    return out.reshape(n, size, size, 3)


def synthetic_page_structure(pages: int = 512, per_page: int = 128, seed: int = 2, duplicated_prefixes: int = 0):
    """The page structure of config C5: `pages` pages of `per_page` regions, page id = idx // per_page.

    Returns (area_percentage f64 [N] on the reference's 0..100 scale (region_processor.py:89-93), page_offs int32
    [pages + 1], names).  Area fractions are seeded log-uniform in [1e-4, 0.2], scaled down where a page would sum to
    more than 1; integer provenance (counter hash), so every box and every rank builds the same table.  Page names have
    distinct first-20-character prefixes (no same-prefix skips, wrc:179-186) except that the first
    `duplicated_prefixes` odd pages repeat the prefix of the page before them."""
    n = pages * per_page
    u = (counter_u64(seed, 0x6100, n) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    frac = np.exp(np.log(1e-4) + u * (np.log(0.2) - np.log(1e-4))).reshape(pages, per_page)
    tot = frac.sum(axis=1, keepdims=True)
    frac = np.where(tot > 1.0, frac / tot, frac)
    names = [f"{p:04d} synthetic page of the C5 set.png" for p in range(pages)]
    for k in range(duplicated_prefixes):
        names[2 * k + 1] = names[2 * k][:20] + f" second scan {k}.png"
    return (frac.reshape(-1) * 100.0), (np.arange(pages + 1, dtype=np.int64) * per_page).astype(np.int32), names


# ---- the reference's own vision-tower geometry --------------------------------------------------
@dataclass(frozen=True)
class TileViTGeometry:
    """Mllama vision tower as the reference's checkpoint configures it (`config.py:58`, transformers
    `configuration_mllama.py:61-82` at image_size 560): <= 4 tiles of 560 x 560, patch 14, 1 + 1600 tokens per tile
    (padded to 1608), 1280-d, 16 heads of 80, MLP 5120, 32 local + 8 gated global layers, the outputs of five
    intermediate layers concatenated to the final one -> 7680-d."""

    image_size: int = 560
    patch_size: int = 14
    num_channels: int = 3
    hidden_size: int = 1280
    num_heads: int = 16
    intermediate_size: int = 5120
    num_layers: int = 32
    num_global_layers: int = 8
    max_num_tiles: int = 4
    max_aspect_ratio_id: int = 8
    intermediate_layers: tuple = (3, 7, 15, 23, 30)
    # "after": index i names the OUTPUT of local layer i (transformers 5.15, what the fixtures pin);
    # "before": the state entering layer i (encoders that record before running a layer; include/mme.h)
    intermediate_save_point: str = "after"
    norm_eps: float = 1e-5

    @property
    def num_patches(self) -> int:  # tokens of a tile, class token included
        return (self.image_size // self.patch_size) ** 2 + 1

    @property
    def padded_patches(self) -> int:
        return (self.num_patches + 7) // 8 * 8

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def patch_dim(self) -> int:
        return self.num_channels * self.patch_size * self.patch_size

    @property
    def output_dim(self) -> int:
        return self.hidden_size * (1 + len(self.intermediate_layers))


TILE_VIT = TileViTGeometry()


def tile_vit_tensor_specs(geom: TileViTGeometry = TILE_VIT):
    """(name, shape, kind, scale) in a fixed order, Hugging Face `MllamaVisionModel` state-dict names."""
    D, F, P, T = geom.hidden_size, geom.intermediate_size, geom.patch_size, geom.max_num_tiles
    A = geom.max_aspect_ratio_id + 1
    emb = D ** -0.5
    specs = [
        ("class_embedding", (D,), "matrix", emb),
        ("patch_embedding.weight", (D, geom.num_channels, P, P), "matrix", 0.02),
        ("gated_positional_embedding.gate", (1,), "gate", 0.6),
        ("gated_positional_embedding.embedding", (geom.num_patches, D), "matrix", emb),
        ("gated_positional_embedding.tile_embedding.weight", (A, T * geom.num_patches * D), "matrix", 0.02),
        ("pre_tile_positional_embedding.gate", (1,), "gate", 0.4),
        ("pre_tile_positional_embedding.embedding.weight", (A, T * D), "matrix", 0.02),
        ("post_tile_positional_embedding.gate", (1,), "gate", -0.5),
        ("post_tile_positional_embedding.embedding.weight", (A, T * D), "matrix", 0.02),
        ("layernorm_pre.weight", (D,), "gamma", 0.02),
        ("layernorm_pre.bias", (D,), "bias", 0.02),
        ("layernorm_post.weight", (D,), "gamma", 0.02),
        ("layernorm_post.bias", (D,), "bias", 0.02),
    ]
    for stack, count, gated in (("transformer", geom.num_layers, False), ("global_transformer", geom.num_global_layers, True)):
        for i in range(count):
            p = f"{stack}.layers.{i}."
            if gated:
                specs += [(p + "gate_attn", (1,), "gate", 0.7853981633974483), (p + "gate_ffn", (1,), "gate", 0.7853981633974483)]
            specs += [
                (p + "self_attn.q_proj.weight", (D, D), "matrix", 0.02),
                (p + "self_attn.k_proj.weight", (D, D), "matrix", 0.02),
                (p + "self_attn.v_proj.weight", (D, D), "matrix", 0.02),
                (p + "self_attn.o_proj.weight", (D, D), "matrix", 0.02),
                (p + "mlp.fc1.weight", (F, D), "matrix", 0.02),
                (p + "mlp.fc1.bias", (F,), "bias", 0.02),
                (p + "mlp.fc2.weight", (D, F), "matrix", 0.02),
                (p + "mlp.fc2.bias", (D,), "bias", 0.02),
                (p + "input_layernorm.weight", (D,), "gamma", 0.02),
                (p + "input_layernorm.bias", (D,), "bias", 0.02),
                (p + "post_attention_layernorm.weight", (D,), "gamma", 0.02),
                (p + "post_attention_layernorm.bias", (D,), "bias", 0.02),
            ]
    return specs


def hashed_normal4(seed: int, stream: int, n: int, start: int = 0) -> np.ndarray:
    """Approximate N(0,1) f32 samples for element counters start .. start+n: the four 16-bit lanes of ONE splitmix64 word
    summed (Irwin-Hall, 4 terms), centred and scaled to unit variance.  Integer provenance like `irwin_hall_normal`,
    a third of its cost -- the vision tower has 860 M parameters to fill."""
    i = np.arange(start, start + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = np.uint64(seed & 0xFFFF) * np.uint64(1 << 48) + np.uint64(stream & 0xFFFFFFFF) * np.uint64(1 << 16)
        w = _splitmix64(_splitmix64(np.uint64(base)) ^ (i * np.uint64(0x2545F4914F6CDD1D)))
    total = (w & np.uint64(0xFFFF)).astype(np.int32)
    for lane in (1, 2, 3):
        total += ((w >> np.uint64(16 * lane)) & np.uint64(0xFFFF)).astype(np.int32)
    # four U{0..65535}: mean 131070, variance 4 * (65536^2 - 1) / 12 -> sigma = 37837.2247...
    return (total - 131070).astype(np.float32) * np.float32(1.0 / 37837.224732)


def make_tile_vit_weights(seed: int = 2, geom: TileViTGeometry = TILE_VIT, threads: int = 8) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of the Mllama vision tower, f32 arrays holding bf16-representable values (the reference
    runs the tower in bf16, embedder.py:78).  A counter-based generator: identical tensors in the build container (where
    they are loaded into transformers' `MllamaVisionModel` to make the golden vectors) and on the GPU box.  Gates (the
    tanh-gated embeddings and the gated global layers) get fixed non-zero values so that every gated path carries data;
    matrices N(0, scale), LayerNorm gamma 1 + N(0, 0.02), biases N(0, 0.02)."""
    from concurrent.futures import ThreadPoolExecutor

    out: dict[str, np.ndarray] = {}
    jobs = []
    step = 1 << 22  # elements per block: bounds the uint64 temporaries and gives the thread pool even work
    for tid, (name, shape, kind, scale) in enumerate(tile_vit_tensor_specs(geom)):
        n = int(np.prod(shape))
        if kind == "gate":
            out[name] = round_to_bf16(np.full(n, scale, dtype=np.float32)).reshape(shape)
            continue
        buf = np.empty(n, dtype=np.float32)
        out[name] = buf.reshape(shape)
        jobs += [(buf, tid, o, min(step, n - o), scale, kind) for o in range(0, n, step)]

    def fill(job):
        buf, tid, o, m, scale, kind = job
        z = hashed_normal4(seed, tid, m, start=o) * np.float32(scale)
        if kind == "gamma":
            z += np.float32(1.0)
        buf[o : o + m] = round_to_bf16(z)

    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(fill, jobs))
    return out


# ---- the reference's language tower: Mllama text model with cross-attention -----------------------
MLLAMA_MAX_SEQ = 128  # positions of the library's rotary table (csrc/mllama_lm.h MLLAMA_MAX_S)
MLLAMA_ROPE_TYPES = ("default", "llama3")  # include/mme.h mme_mllama_lm_weights.rope_type: the index


@dataclass(frozen=True)
class MllamaLMGeometry:
    """`MllamaTextConfig` + the projector's input width, as intfloat/mmE5-mllama-11b-instruct configures them: 4096-d, 32 heads
    of 128 over 8 KV heads, MLP 14336, 40 layers of which 3, 8, ..., 38 cross-attend the image, llama3 rotary frequencies.
    `cross_attention_layers` may name indices at or beyond `num_layers` (a stack cut short keeps the tuple): they are ignored."""

    hidden_size: int = 4096
    num_heads: int = 32
    num_kv_heads: int = 8
    intermediate_size: int = 14336
    num_layers: int = 40
    cross_attention_layers: tuple = (3, 8, 13, 18, 23, 28, 33, 38)
    vocab_size: int = 128256
    vision_output_dim: int = 7680
    image_token_id: int = 128256
    rms_norm_eps: float = 1e-5
    hidden_act: str = "silu"
    rope_type: str = "llama3"
    rope_theta: float = 500000.0
    rope_factor: float = 8.0
    rope_low_freq_factor: float = 1.0
    rope_high_freq_factor: float = 4.0
    rope_original_max: int = 8192

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads

    @property
    def embed_rows(self) -> int:  # embed_tokens holds vocab_size + 8 rows (<|image|> among the extra ones)
        return self.vocab_size + 8

    @property
    def cross_layers(self) -> tuple:
        return tuple(int(i) for i in self.cross_attention_layers if 0 <= int(i) < self.num_layers)


MLLAMA_LM_11B = MllamaLMGeometry()
SUPPORTED_MLLAMA_LM = {"head_dim": (128,), "heads / kv_heads": (1, 2, 4, 8), "intermediate_size": "a multiple of 64 up to 16384", "num_layers": "1..64",
                       "vocab_size": "vocab_size + 8 <= 2^18", "vision_output_dim": "a multiple of 64 up to 8192", "hidden_act": ("silu",),
                       "rope_type": MLLAMA_ROPE_TYPES}


def mllama_lm_geometry_problem(geom: MllamaLMGeometry):
    """None, or why the library refuses `geom` (the text names the field, the value found and the supported set)."""
    if geom.num_heads < 1 or geom.num_heads > 64 or geom.hidden_size != geom.num_heads * 128:
        return f"hidden_size = {geom.hidden_size} at num_heads = {geom.num_heads}; supported: 1..64 heads of 128"
    if geom.num_kv_heads < 1 or geom.num_heads % geom.num_kv_heads or geom.num_heads // geom.num_kv_heads not in (1, 2, 4, 8):
        return f"num_kv_heads = {geom.num_kv_heads} at num_heads = {geom.num_heads}; supported: heads / kv_heads in (1, 2, 4, 8)"
    if geom.intermediate_size < 64 or geom.intermediate_size % 64 or geom.intermediate_size > 16384:
        return f"intermediate_size = {geom.intermediate_size}; supported: a multiple of 64 up to 16384"
    if not 1 <= geom.num_layers <= 64:
        return f"num_layers = {geom.num_layers}; supported: 1..64"
    cross = tuple(geom.cross_attention_layers)
    if any(b <= a for a, b in zip(cross, cross[1:])) or any(i < 0 for i in cross):
        return f"cross_attention_layers = {cross}; supported: strictly increasing, non-negative"
    if geom.vocab_size < 1 or geom.vocab_size + 8 > 1 << 18:
        return f"vocab_size = {geom.vocab_size}; supported: vocab_size + 8 <= 2^18"
    if geom.vision_output_dim < 64 or geom.vision_output_dim % 64 or geom.vision_output_dim > 8192:
        return f"vision_output_dim = {geom.vision_output_dim}; supported: a multiple of 64 up to 8192"
    if not 0 <= geom.image_token_id < geom.embed_rows:
        return f"image_token_id = {geom.image_token_id}; supported: 0..vocab_size + 7"
    if geom.hidden_act != "silu":
        return f"hidden_act = {geom.hidden_act!r}; supported: 'silu'"
    if geom.rope_type not in MLLAMA_ROPE_TYPES:
        return f"rope_type = {geom.rope_type!r}; supported: {MLLAMA_ROPE_TYPES}"
    return None


def mllama_lm_tensor_specs(geom: MllamaLMGeometry = MLLAMA_LM_11B):
    """(name, shape, kind, scale) in a fixed order: the names of transformers 5.15's `MllamaForConditionalGeneration` state dict
    without the leading `model.`.  The scales give attention logits and residual branches of order one at every width."""
    D, KV, I = geom.hidden_size, geom.num_kv_heads * 128, geom.intermediate_size
    qk, lin, down = 1.3 * D ** -0.5, D ** -0.5, I ** -0.5
    specs = [
        ("language_model.embed_tokens.weight", (geom.embed_rows, D), "matrix", 1.0),
        ("language_model.norm.weight", (D,), "gamma", 0.25),
        ("multi_modal_projector.weight", (D, geom.vision_output_dim), "matrix", geom.vision_output_dim ** -0.5),
        ("multi_modal_projector.bias", (D,), "matrix", 0.5),
    ]
    cross = set(geom.cross_layers)
    for i in range(geom.num_layers):
        p = f"language_model.layers.{i}."
        specs += [(p + "input_layernorm.weight", (D,), "gamma", 0.25), (p + "post_attention_layernorm.weight", (D,), "gamma", 0.25)]
        if i in cross:
            a = p + "cross_attn."
            # q / k three times the unit scale: without q_norm / k_norm the logits would be three times as large
            specs += [(a + "q_proj.weight", (D, D), "matrix", 3 * lin), (a + "k_proj.weight", (KV, D), "matrix", 3 * lin), (a + "v_proj.weight", (KV, D), "matrix", lin),
                      (a + "o_proj.weight", (D, D), "matrix", lin), (a + "q_norm.weight", (128,), "gamma", 0.25), (a + "k_norm.weight", (128,), "gamma", 0.25),
                      (p + "cross_attn_attn_gate", (1,), "gate", 0.9), (p + "cross_attn_mlp_gate", (1,), "gate", -1.5)]
        else:
            a = p + "self_attn."
            specs += [(a + "q_proj.weight", (D, D), "matrix", qk), (a + "k_proj.weight", (KV, D), "matrix", qk), (a + "v_proj.weight", (KV, D), "matrix", lin),
                      (a + "o_proj.weight", (D, D), "matrix", lin)]
        specs += [(p + "mlp.gate_proj.weight", (I, D), "matrix", lin), (p + "mlp.up_proj.weight", (I, D), "matrix", lin),
                  (p + "mlp.down_proj.weight", (D, I), "matrix", down)]
    return specs


def make_mllama_lm_weights(seed: int = 7, geometry: MllamaLMGeometry = MLLAMA_LM_11B, threads: int = 8) -> dict[str, np.ndarray]:
    """Seeded synthetic weights of the language tower and the projector, f32 arrays of bf16-representable values, from the
    counter-based generator of `make_tile_vit_weights`.  The gates are NON-ZERO (a checkpoint's are; a zero gate would switch
    the cross layers off) and the norm weights are 1 + N(0, 0.25), so that a dropped norm weight or gate changes the output."""
    from concurrent.futures import ThreadPoolExecutor

    out: dict[str, np.ndarray] = {}
    jobs = []
    step = 1 << 22
    for tid, (name, shape, kind, scale) in enumerate(mllama_lm_tensor_specs(geometry)):
        n = int(np.prod(shape))
        if kind == "gate":
            out[name] = round_to_bf16(np.full(n, scale, dtype=np.float32)).reshape(shape)
            continue
        buf = np.empty(n, dtype=np.float32)
        out[name] = buf.reshape(shape)
        jobs += [(buf, tid, o, min(step, n - o), scale, kind) for o in range(0, n, step)]

    def fill(job):
        buf, tid, o, m, scale, kind = job
        z = hashed_normal4(seed, tid, m, start=o) * np.float32(scale)
        if kind == "gamma":
            z += np.float32(1.0)
        buf[o : o + m] = round_to_bf16(z)

    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(fill, jobs))
    return out


def infer_mllama_lm_geometry(w: dict, **config) -> MllamaLMGeometry:
    """The geometry the tensor shapes of a canonical-name dict say; what no shape says (the rotary parameters, eps, the image
    token, which default to the 11B checkpoint's except image_token_id = vocab_size) comes from `config`."""
    rows, D = np.shape(w["language_model.embed_tokens.weight"])
    layers = _layer_count(w, "language_model.layers.{}.input_layernorm.weight")
    cross = tuple(i for i in range(layers) if f"language_model.layers.{i}.cross_attn.q_proj.weight" in w)
    some = f"language_model.layers.{cross[0]}.cross_attn." if cross else "language_model.layers.0.self_attn."
    kv = int(np.shape(w[some + "k_proj.weight"])[0])
    vocab = int(rows) - 8
    fields = dict(hidden_size=int(D), num_heads=int(D) // 128, num_kv_heads=kv // 128, num_layers=layers, cross_attention_layers=cross, vocab_size=vocab,
                  intermediate_size=int(np.shape(w["language_model.layers.0.mlp.gate_proj.weight"])[0]),
                  vision_output_dim=int(np.shape(w["multi_modal_projector.weight"])[1]), image_token_id=vocab)
    fields.update(config)
    return MllamaLMGeometry(**fields)


def mllama_rope_inv_freq(geom: MllamaLMGeometry) -> np.ndarray:
    """transformers' rotary inverse frequencies f32 [64] for `geom` (modeling_rope_utils.py: the default rule, and llama3's
    three bands: wavelengths under original_max / high_freq_factor kept, over original_max / low_freq_factor divided by
    `factor`, between the two interpolated), in f32 arithmetic as torch forms them."""
    f32 = np.float32
    inv = (f32(1.0) / np.power(f32(geom.rope_theta), np.arange(0, 128, 2, dtype=np.int64).astype(f32) / f32(128))).astype(f32)
    if geom.rope_type == "default":
        return inv
    orig, low, high, factor = f32(geom.rope_original_max), f32(geom.rope_low_freq_factor), f32(geom.rope_high_freq_factor), f32(geom.rope_factor)
    wavelen = f32(2.0 * np.pi) / inv
    inv_l = np.where(wavelen > orig / low, inv / factor, inv).astype(f32)
    smooth = (orig / wavelen - low) / (high - low)
    smoothed = ((f32(1.0) - smooth) * inv_l / factor + smooth * inv_l).astype(f32)
    medium = ~(wavelen < orig / high) & ~(wavelen > orig / low)
    return np.where(medium, smoothed, inv_l).astype(f32)


def mllama_rope_tables(geom: MllamaLMGeometry, positions: int = MLLAMA_MAX_SEQ):
    """(cos, sin) f32 [positions, 64]: the angle position * inv_freq formed in f32, as the library's host code builds its table."""
    ang = (np.arange(positions, dtype=np.float32)[:, None] * mllama_rope_inv_freq(geom)[None, :]).astype(np.float32)
    return np.cos(ang.astype(np.float64)).astype(np.float32), np.sin(ang.astype(np.float64)).astype(np.float32)
