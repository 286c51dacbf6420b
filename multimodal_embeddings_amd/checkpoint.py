"""Read an encoder checkpoint from a LOCAL directory (host only; nothing here touches the network or a GPU).

The reference names its encoder and lets `from_pretrained` fetch it (deprecated_package/embedder.py:73-82).  This engine
never fetches: `read_checkpoint(path, encoder)` takes a directory that is already on disk --

    config.json  [+ preprocessor_config.json]
    model.safetensors  |  model.safetensors.index.json + shards  |  pytorch_model.bin

-- checks that its configuration is a geometry the library is built for ("vit_b16": exactly ViT-B/16; "vit": any of the
supported ViT/16 and ViT/32 @224 family, `weights.SUPPORTED_VIT`, read from config.json; "clip": a CLIP image tower of that family,
`CLIPVisionModel[WithProjection]` or the vision half of a whole `CLIPModel`; "clip_text": a CLIP text tower,
`CLIPTextModel[WithProjection]` or the text half of a whole `CLIPModel`; "dinov2": a DINOv2 ViT/14 image tower (`Dinov2Model`:
257 tokens at 224 pixels, LayerScale; the checkpoint's position table is interpolated to 16 x 16 here, once); "siglip": a SigLIP ViT/16 @224 image tower with its
attention-pooling head, `SiglipVisionModel` or the vision half of a whole `SiglipModel`; "mllama_tiles": the tile tower), maps the tensor names to the canonical ones
(`weights.vit_tensor_specs()` / `weights.tile_vit_tensor_specs()`) and returns the tensors IN THE FILE'S OWN DTYPE: a
bf16 checkpoint stays bf16 on the host, and `Engine.load_vit_checkpoint` / `load_tile_vit_checkpoint` hand the raw
bytes to the device, where they are converted and folded (csrc/weight_load.hip: DevPrep; kernels in csrc/weight_prep.hip).

    python -m multimodal_embeddings_amd.checkpoint DIR [--encoder vit_b16|vit|clip|mllama_tiles|clip_text|siglip_vit|siglip_text|dinov2]

prints what a load would find (dtype, geometry, mean / std, tensor count, bytes): the offline "will this load" check.
"""
from __future__ import annotations

import dataclasses
import json
import logging
import os
import re
from dataclasses import dataclass, field

from . import config
from ._lib import MmeError, ResizeSpec
from .weights import (CLIP_B16, CLIP_TEXT_B, DINOV2_B14, SIGLIP_B16, SIGLIP_LOGIT_KEYS, SIGLIP_TEXT_B, TILE_VIT, VIT_B16, CLIPGeometry, CLIPTextGeometry,
                      Dinov2Geometry, SiglipGeometry, SiglipTextGeometry, TileViTGeometry, ViTGeometry, clip_geometry_problem, clip_text_geometry_problem,
                      dinov2_geometry_problem, siglip_geometry_problem, siglip_text_geometry_problem, vit_geometry_problem)

logger = logging.getLogger("multimodal_embeddings_amd")

ENCODERS = ("vit_b16", "vit", "clip", "mllama_tiles", "clip_text", "siglip", "siglip_text", "dinov2", "mllama_text")
# The command line below and RegionEmbedder spell the SigLIP tower "siglip_vit": both have always refused the bare name
# "siglip" as an unknown encoder and keep doing so; read_checkpoint, Checkpoint.encoder and the Engine say "siglip".
SIGLIP_ALIAS = "siglip_vit"
CLI_ENCODERS = tuple(SIGLIP_ALIAS if e == "siglip" else e for e in ENCODERS)
VIT_ENCODERS = ("vit_b16", "vit")  # one loader, one tensor layout; "vit" takes its geometry from config.json
SUPPORTED_ASPECT_RATIOS = [[1, 1], [1, 2], [1, 3], [1, 4], [2, 1], [2, 2], [3, 1], [4, 1]]
_DTYPE_IDS = {"float32": 0, "bfloat16": 1, "float16": 2}  # include/mme.h MME_DT_*
_warned_resize_rule = False


@dataclass
class Checkpoint:
    encoder: str
    tensors: dict            # canonical name -> contiguous torch tensor in the file's own dtype (shape as the specs list it)
    dtype: str               # "float32" | "bfloat16" | "float16"
    geometry: object         # ViTGeometry | TileViTGeometry
    image_mean: tuple | None = None
    image_std: tuple | None = None
    resize_spec: object = None  # the ResizeSpec of preprocessor_config.json, read under resize_rule = "checkpoint" only
    source: list = field(default_factory=list)  # files read
    extra: dict = field(default_factory=dict)   # "dinov2": {"position_table": f32 [257, D], the interpolated table the device holds}

    @property
    def dtype_id(self) -> int:
        return _DTYPE_IDS[self.dtype]

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors.values())


# ---- the decision RegionEmbedder takes on `model_name` (no GPU needed) ---------------------------------------------------
def resolve_model_source(model_name, weights=None, allow_synthetic: bool = True) -> str:
    """-> "weights" (the caller's dict wins), "checkpoint" (`model_name` is an existing directory) or "synthetic"
    (seeded weights; one WARNING says so, except for config.DEFAULT_MODEL_NAME, which says it itself).  With
    `allow_synthetic=False` a name that is no directory raises."""
    if weights is not None:
        return "weights"
    if isinstance(model_name, (str, os.PathLike)) and os.path.isdir(model_name):
        return "checkpoint"
    if not allow_synthetic:
        raise MmeError(f"model_name={model_name!r} is not a local checkpoint directory; this engine never fetches "
                       "(pass a directory holding config.json + model.safetensors, or weights=...)")
    if model_name == config.DEFAULT_MODEL_NAME:
        return "synthetic"
    logger.warning(f"model_name={model_name!r} is not a local checkpoint directory and this engine never fetches: the encoder runs on "
                   "SEEDED SYNTHETIC weights (pass a checkpoint directory, or allow_synthetic=False to make this an error)")
    return "synthetic"


# ---- names --------------------------------------------------------------------------------------------------------------
_VIT_LEGACY = (
    (re.compile(r"^encoder\.layer\.(\d+)\.attention\.attention\.query\.(weight|bias)$"), r"layers.\1.attention.q_proj.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.attention\.attention\.key\.(weight|bias)$"), r"layers.\1.attention.k_proj.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.attention\.attention\.value\.(weight|bias)$"), r"layers.\1.attention.v_proj.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.attention\.output\.dense\.(weight|bias)$"), r"layers.\1.attention.o_proj.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.intermediate\.dense\.(weight|bias)$"), r"layers.\1.mlp.fc1.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.output\.dense\.(weight|bias)$"), r"layers.\1.mlp.fc2.\2"),
    (re.compile(r"^encoder\.layer\.(\d+)\.(layernorm_before|layernorm_after)\.(weight|bias)$"), r"layers.\1.\2.\3"),
)


def canonical_vit_name(key: str):
    """Checkpoint key -> canonical name, or None for a key the encoder does not use (pooler, classifier)."""
    if key.startswith("vit."):
        key = key[4:]
    if key.startswith(("pooler.", "classifier.")):
        return None
    for pat, rep in _VIT_LEGACY:
        if pat.match(key):
            return pat.sub(rep, key)
    return key


def canonical_clip_name(key: str):
    """Checkpoint key -> canonical name (`weights.clip_tensor_specs`: the keys of `CLIPVisionModelWithProjection`), or None
    for what the image tower does not use: the text tower, text_projection, logit_scale, the position_ids buffers."""
    if key.startswith(("text_model.", "text_projection.")) or key == "logit_scale" or key.endswith(".position_ids"):
        return None
    # CLIPVisionModel.save_pretrained of transformers 5 writes the tower's own keys, without the "vision_model." prefix
    if key.startswith(("embeddings.", "pre_layrnorm.", "encoder.layers.", "post_layernorm.")):
        return "vision_model." + key
    return key


def canonical_clip_text_name(key: str):
    """Checkpoint key -> canonical name (`weights.clip_text_tensor_specs`: the keys of `CLIPTextModelWithProjection`), or None
    for what the text tower does not use: the image tower, visual_projection, logit_scale, the position_ids buffers."""
    if key.startswith(("vision_model.", "visual_projection.")) or key == "logit_scale" or key.endswith(".position_ids"):
        return None
    # CLIPTextModel.save_pretrained of transformers 5 writes the tower's own keys, without the "text_model." prefix
    if key.startswith(("embeddings.", "encoder.layers.", "final_layer_norm.")):
        return "text_model." + key
    return key


def canonical_siglip_name(key: str):
    """Checkpoint key -> canonical name (`weights.siglip_tensor_specs`: the vision keys of a `SiglipModel`), or None for what
    the image tower does not use: the text tower, logit_scale, logit_bias, the position_ids buffers."""
    if key.startswith("text_model.") or key in ("logit_scale", "logit_bias") or key.endswith(".position_ids"):
        return None
    # SiglipVisionModel.save_pretrained of transformers 5 writes the tower's own keys, without the "vision_model." prefix
    if key.startswith(("embeddings.", "encoder.layers.", "post_layernorm.", "head.")):
        return "vision_model." + key
    return key


DINOV2_POSITIONS = "embeddings.position_embeddings"


def canonical_dinov2_name(key: str):
    """Checkpoint key -> canonical name (`weights.dinov2_tensor_specs`: the keys of `Dinov2Model`), or None for what the tower
    does not use: mask_token (read past), a classifier head."""
    if key.startswith("dinov2."):  # Dinov2ForImageClassification / Dinov2Backbone keep the model under this prefix
        key = key[7:]
    if key.startswith("classifier.") or key == "embeddings.mask_token":
        return None
    return key


def interpolate_dinov2_positions(table):
    """The checkpoint's position table [1, 1 + g * g, D] (torch, any float type) -> f32 [257, D] for 224 x 224 pixels at patch 14:
    what `Dinov2Embeddings.interpolate_pos_encoding` returns on every forward of an f32 model, bit for bit, computed once.  A
    257-row table is taken as it is; else the class row is kept and the g x g patch grid goes through the model's own call,
    `F.interpolate(f32, size=(16, 16), mode="bicubic", align_corners=False)`.  A patch part that is no square grid is refused."""
    import torch

    t = table.reshape(-1, table.shape[-1]).to(torch.float32)
    rows, D = int(t.shape[0]), int(t.shape[1])
    g = int(round((rows - 1) ** 0.5))
    if rows < 2 or g * g != rows - 1:
        raise MmeError(f"tensor {DINOV2_POSITIONS!r} has {rows} rows: the patch part ({rows - 1} rows) is no square grid")
    if g == 16:
        return t.contiguous()
    patch = t[1:].reshape(1, g, g, D).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch, size=(16, 16), mode="bicubic", align_corners=False)
    return torch.cat((t[:1], patch.permute(0, 2, 3, 1).reshape(256, D)), dim=0).contiguous()


def canonical_siglip_text_name(key: str):
    """Checkpoint key -> canonical name (`weights.siglip_text_tensor_specs`: the text keys of a `SiglipModel`, and its two
    scalars `logit_scale` / `logit_bias`), or None for what the text tower does not use: the image tower, the position_ids buffers."""
    if key.startswith("vision_model.") or key.endswith(".position_ids"):
        return None
    # SiglipTextModel.save_pretrained of transformers 5 writes the tower's own keys, without the "text_model." prefix
    if key.startswith(("embeddings.", "encoder.layers.", "final_layer_norm.", "head.")):
        return "text_model." + key
    return key


def canonical_tile_name(key: str):
    """Checkpoint key -> canonical name, or None for a key outside the vision tower."""
    for prefix in ("model.vision_model.", "vision_model."):
        if key.startswith(prefix):
            return key[len(prefix):]
    if key.startswith(("model.", "language_model.", "multi_modal_projector.", "lm_head.")):
        return None
    return key


def canonical_mllama_lm_name(key: str):
    """Checkpoint key -> canonical name (weights.mllama_lm_tensor_specs: `language_model.…`, `multi_modal_projector.…`), or None for
    a key outside the language tower and the projector.  transformers 5 spells the tensors `model.language_model.…` and
    `model.multi_modal_projector.…`; checkpoints saved by 4.4x (mmE5's) `language_model.model.…` and `multi_modal_projector.…`.
    `lm_head` is not read."""
    if key.startswith("model."):
        key = key[len("model."):]
    if key.startswith("language_model.model."):
        return "language_model." + key[len("language_model.model."):]
    if key.startswith("language_model.lm_head.") or key.startswith("lm_head."):
        return None
    if key.startswith(("language_model.", "multi_modal_projector.")):
        return key
    return None


# ---- configuration ------------------------------------------------------------------------------------------------------
def _load_json(path):
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f)


def _expect(cfg: dict, fld: str, built, where: str, default=None):
    found = cfg.get(fld, default)
    same = found == built
    if isinstance(built, float) and isinstance(found, (int, float)):
        same = abs(float(found) - built) <= 1e-12 * max(1.0, abs(built))
    if not same:
        raise MmeError(f"{where}: {fld} = {found!r}, but this library is built for {fld} = {built!r}")


# Every function below is an `encoders.Encoder.config_geometry`: (config.json as a dict, the directory) -> (geometry, where the
# tower's fields were found, for the messages).  A whole two-tower model keeps them under vision_config / text_config.
def _sub_config(cfg: dict, key: str):
    if key in cfg:
        return dict(cfg[key]), f"config.json: {key}"
    return cfg, "config.json"


def _ints(cfg: dict, where: str, fields: dict) -> dict:
    """cfg's value of every field (`fields`: name -> default, None where the file must name it), each an integer or refused."""
    out = {}
    for fld, default in fields.items():
        out[fld] = cfg.get(fld, default)
        if not isinstance(out[fld], int) or isinstance(out[fld], bool):
            raise MmeError(f"{where}: {fld} = {out[fld]!r}; an integer is required")
    return out


def _refuse(bad, where: str):
    """Raises for a `*_geometry_problem` finding, under the name config.json gives the field."""
    if bad:
        names = {"num_layers": "num_hidden_layers", "num_heads": "num_attention_heads"}
        raise MmeError(f"{where}: {names.get(bad[0], bad[0])} = {bad[1]!r}; supported: {bad[2]}")


def _image_fields(cfg: dict, where: str, b) -> dict:
    """The ViTGeometry arguments of an image tower's config: the six sizes required as integers, the rest defaulting to b's."""
    v = _ints(cfg, where, dict.fromkeys(("image_size", "patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")))
    return dict(image_size=v["image_size"], patch_size=v["patch_size"], num_channels=cfg.get("num_channels", b.num_channels), hidden_size=v["hidden_size"],
                num_layers=v["num_hidden_layers"], num_heads=v["num_attention_heads"], intermediate_size=v["intermediate_size"],
                layer_norm_eps=float(cfg.get("layer_norm_eps", b.layer_norm_eps)))


def _text_fields(cfg: dict, where: str, b, token_id: str) -> dict:
    """The arguments the two text geometries share; a field the file leaves out has b's value, as transformers reads it."""
    v = _ints(cfg, where, {"hidden_size": b.hidden_size, "num_hidden_layers": b.num_layers, "num_attention_heads": b.num_heads,
                           "intermediate_size": b.intermediate_size, "vocab_size": b.vocab_size, "max_position_embeddings": b.max_position_embeddings,
                           token_id: getattr(b, token_id)})
    return dict(hidden_size=v["hidden_size"], num_layers=v["num_hidden_layers"], num_heads=v["num_attention_heads"], intermediate_size=v["intermediate_size"],
                vocab_size=v["vocab_size"], max_position_embeddings=v["max_position_embeddings"], hidden_act=cfg.get("hidden_act", b.hidden_act),
                layer_norm_eps=float(cfg.get("layer_norm_eps", b.layer_norm_eps)), **{token_id: v[token_id]})


def _vit_geometry(cfg: dict, path: str):
    g, where = VIT_B16, "config.json"
    for fld, built in (("image_size", g.image_size), ("patch_size", g.patch_size), ("hidden_size", g.hidden_size),
                       ("num_hidden_layers", g.num_layers), ("num_attention_heads", g.num_heads), ("intermediate_size", g.intermediate_size),
                       ("num_channels", g.num_channels)):
        _expect(cfg, fld, built, where, default=built if fld == "num_channels" else None)
    _expect(cfg, "hidden_act", "gelu", where)
    _expect(cfg, "qkv_bias", True, where, default=True)
    return ViTGeometry(layer_norm_eps=float(cfg.get("layer_norm_eps", g.layer_norm_eps))), where


def _vit_family_geometry(cfg: dict, path: str):
    """config.json of any ViT/16 or ViT/32 @224 the engine runs (weights.SUPPORTED_VIT); a field outside the set is refused with the
    field, the value found and the supported values."""
    where = "config.json"
    g = ViTGeometry(**_image_fields(cfg, where, VIT_B16))
    _refuse(vit_geometry_problem(g), where)
    _expect(cfg, "hidden_act", "gelu", where)
    _expect(cfg, "qkv_bias", True, where, default=True)
    return g, where


def _clip_geometry(cfg: dict, path: str):
    """The vision configuration of a CLIP checkpoint (CLIPVisionConfig) -> geometry; the same supported set as "vit", plus
    hidden_act and projection_dim.  A whole CLIP config names projection_dim at its top level; whether the checkpoint has a
    visual_projection at all is decided by its tensors (`_optional_projection`)."""
    vcfg, where = _sub_config(cfg, "vision_config")
    if vcfg is not cfg and "projection_dim" in cfg:
        vcfg["projection_dim"] = cfg["projection_dim"]
    g = CLIPGeometry(**_image_fields(vcfg, where, CLIP_B16), projection_dim=vcfg.get("projection_dim"), hidden_act=vcfg.get("hidden_act", CLIP_B16.hidden_act))
    _refuse(clip_geometry_problem(g), where)
    return g, where


def _siglip_geometry(cfg: dict, path: str):
    """The vision configuration of a SigLIP checkpoint (SiglipVisionConfig) -> geometry: patch 16 at 224 pixels, heads of 64,
    `gelu_pytorch_tanh`, the pooling head.  A field the file leaves out has SiglipVisionConfig's default, except the sizes."""
    vcfg, where = _sub_config(cfg, "vision_config")
    g = SiglipGeometry(**_image_fields(vcfg, where, SIGLIP_B16), hidden_act=vcfg.get("hidden_act", SIGLIP_B16.hidden_act),
                       vision_use_head=vcfg.get("vision_use_head", True))
    _refuse(siglip_geometry_problem(g), where)
    return g, where


def _dinov2_geometry(cfg: dict, path: str):
    """config.json of a DINOv2 checkpoint (Dinov2Config) -> geometry.  `image_size` there (518 for the released models) only
    sizes the position table, which is read off the tensor; the engine runs 224 pixels.  A field the file leaves out has
    Dinov2Config's default, except the sizes."""
    b, where = DINOV2_B14, "config.json"
    if "registers" in str(cfg.get("model_type", "")) or cfg.get("num_register_tokens", 0) not in (0, None):
        raise MmeError(f"{where}: model_type = {cfg.get('model_type')!r}, num_register_tokens = {cfg.get('num_register_tokens', 0)!r}; supported: "
                       "dinov2 with num_register_tokens = 0 (Dinov2WithRegisters is not run)")
    v = _ints(cfg, where, dict.fromkeys(("patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads")))
    ratio = cfg.get("mlp_ratio", 4)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or ratio <= 0:
        raise MmeError(f"{where}: mlp_ratio = {ratio!r}; a positive number is required")
    F = int(v["hidden_size"] * ratio)
    g = Dinov2Geometry(patch_size=v["patch_size"], num_channels=cfg.get("num_channels", b.num_channels), hidden_size=v["hidden_size"],
                       num_layers=v["num_hidden_layers"], num_heads=v["num_attention_heads"], intermediate_size=F,
                       layer_norm_eps=float(cfg.get("layer_norm_eps", b.layer_norm_eps)), hidden_act=cfg.get("hidden_act", b.hidden_act),
                       use_swiglu_ffn=cfg.get("use_swiglu_ffn", False))
    bad = dinov2_geometry_problem(g)
    if bad and bad[0] == "intermediate_size":
        raise MmeError(f"{where}: mlp_ratio = {ratio!r} at hidden_size = {g.hidden_size} (an MLP of {F}); supported: mlp_ratio x hidden_size {bad[2]}")
    _refuse(bad, where)
    _expect(cfg, "qkv_bias", True, where, default=True)
    return g, where


def _clip_text_geometry(cfg: dict, path: str):
    """The text configuration of a CLIP checkpoint (CLIPTextConfig) -> geometry.  A field the file leaves out has
    CLIPTextConfig's default (clip-vit-base-patch16's text tower), as transformers reads it."""
    tcfg, where = _sub_config(cfg, "text_config")
    if tcfg is not cfg:  # a whole CLIP model: projection_dim sits at the top level, CLIPConfig's own field and default
        tcfg["projection_dim"] = cfg.get("projection_dim", CLIP_TEXT_B.projection_dim)
    g = CLIPTextGeometry(**_text_fields(tcfg, where, CLIP_TEXT_B, "eos_token_id"), projection_dim=tcfg.get("projection_dim"))
    _refuse(clip_text_geometry_problem(g), where)
    return g, where


def _siglip_text_geometry(cfg: dict, path: str):
    """The text configuration of a SigLIP checkpoint (SiglipTextConfig) -> geometry.  A field the file leaves out has
    SiglipTextConfig's default (siglip-base-patch16-224's text tower; projection_size: hidden_size), as transformers reads it."""
    tcfg, where = _sub_config(cfg, "text_config")
    if tcfg is cfg and cfg.get("model_type") == "siglip_vision_model":
        raise MmeError(f"{path}: config.json has model_type = 'siglip_vision_model': the directory holds no text tower")
    if "naflex" in str(cfg.get("model_type", "")).lower() or "naflex" in str(tcfg.get("model_type", "")).lower():
        raise MmeError(f"{where}: model_type = {cfg.get('model_type')!r}; supported: siglip, siglip_text_model (the NaFlex variants are not run)")
    fields = _text_fields(tcfg, where, SIGLIP_TEXT_B, "pad_token_id")
    proj = tcfg.get("projection_size")
    g = SiglipTextGeometry(**fields, projection_size=fields["hidden_size"] if proj is None else proj)
    _refuse(siglip_text_geometry_problem(g), where)
    return g, where


def _tile_geometry(cfg: dict, path: str):
    cfg, where = _sub_config(cfg, "vision_config")  # a whole Mllama model keeps the tower's fields there
    g = TILE_VIT
    for fld, built in (("image_size", g.image_size), ("patch_size", g.patch_size), ("hidden_size", g.hidden_size),
                       ("attention_heads", g.num_heads), ("intermediate_size", g.intermediate_size), ("max_num_tiles", g.max_num_tiles)):
        _expect(cfg, fld, built, where)
    _expect(cfg, "num_channels", g.num_channels, where, default=g.num_channels)
    _expect(cfg, "hidden_act", "gelu", where)
    ratios = cfg.get("supported_aspect_ratios")
    if [list(r) for r in (ratios or [])] != SUPPORTED_ASPECT_RATIOS:
        raise MmeError(f"{where}: supported_aspect_ratios = {ratios!r}, but this library is built for supported_aspect_ratios = {SUPPORTED_ASPECT_RATIOS!r}")
    for fld in ("num_hidden_layers", "num_global_layers", "intermediate_layers_indices"):
        if fld not in cfg:
            raise MmeError(f"{where}: {fld} is missing")
    return TileViTGeometry(num_layers=int(cfg["num_hidden_layers"]), num_global_layers=int(cfg["num_global_layers"]),
                           intermediate_layers=tuple(int(v) for v in cfg["intermediate_layers_indices"]),
                           norm_eps=float(cfg.get("norm_eps", g.norm_eps))), where


def _mllama_lm_geometry(cfg: dict, path: str):
    """text_config of a whole Mllama model (+ vision_config.vision_output_dim and image_token_index) -> MllamaLMGeometry.  The
    rotary parameters are `rope_parameters` (transformers 5) or `rope_scaling` + `rope_theta` (4.4x)."""
    from .weights import MLLAMA_LM_11B, MllamaLMGeometry, mllama_lm_geometry_problem

    b = MLLAMA_LM_11B
    if "text_config" not in cfg:
        raise MmeError("config.json: text_config is missing (supported: the config of a whole MllamaForConditionalGeneration)")
    t, where = dict(cfg["text_config"]), "config.json: text_config"
    v = _ints(t, where, {"hidden_size": b.hidden_size, "num_attention_heads": b.num_heads, "num_key_value_heads": b.num_kv_heads,
                         "intermediate_size": b.intermediate_size, "num_hidden_layers": b.num_layers, "vocab_size": b.vocab_size})
    rope = dict(t.get("rope_parameters") or t.get("rope_scaling") or {})
    rope_type = rope.get("rope_type", rope.get("type", "default"))
    theta = rope.get("rope_theta", t.get("rope_theta", b.rope_theta))
    vision = _ints(dict(cfg.get("vision_config") or {}), "config.json: vision_config", {"vision_output_dim": b.vision_output_dim})
    top = _ints(cfg, "config.json", {"image_token_index": v["vocab_size"]})
    cross = t.get("cross_attention_layers", list(b.cross_attention_layers))
    if not isinstance(cross, (list, tuple)) or not all(isinstance(i, int) and not isinstance(i, bool) for i in cross):
        raise MmeError(f"{where}: cross_attention_layers = {cross!r}; a list of integers is required")
    g = MllamaLMGeometry(hidden_size=v["hidden_size"], num_heads=v["num_attention_heads"], num_kv_heads=v["num_key_value_heads"],
                         intermediate_size=v["intermediate_size"], num_layers=v["num_hidden_layers"], cross_attention_layers=tuple(cross),
                         vocab_size=v["vocab_size"], vision_output_dim=vision["vision_output_dim"], image_token_id=top["image_token_index"],
                         rms_norm_eps=float(t.get("rms_norm_eps", b.rms_norm_eps)), hidden_act=t.get("hidden_act", b.hidden_act), rope_type=rope_type,
                         rope_theta=float(theta), rope_factor=float(rope.get("factor", b.rope_factor)),
                         rope_low_freq_factor=float(rope.get("low_freq_factor", b.rope_low_freq_factor)),
                         rope_high_freq_factor=float(rope.get("high_freq_factor", b.rope_high_freq_factor)),
                         rope_original_max=int(rope.get("original_max_position_embeddings", b.rope_original_max)))
    bad = mllama_lm_geometry_problem(g)
    if bad:
        raise MmeError(f"{where}: {bad}")
    return g, where


RESIZE_RULES = ("fit_pad", "clip")  # _lib.Engine.RESIZE_RULES / MME_RESIZE_* (include/mme.h)
CLIP_RULE_ENCODERS = ("vit_b16", "vit", "clip", "siglip", "dinov2")  # the single-tile encoders K1's "clip" rule feeds


def check_resize_rule(resize_rule, encoder: str):
    """None -> "fit_pad"; "checkpoint" and a ResizeSpec pass as they are; raises for an unknown rule and for "clip",
    "checkpoint" or a ResizeSpec with the tile encoder."""
    rule = "fit_pad" if resize_rule is None else resize_rule
    if isinstance(rule, ResizeSpec) or rule == "checkpoint":
        if encoder not in CLIP_RULE_ENCODERS:
            raise MmeError(f"resize_rule = {resize_rule!r} (a resize of the whole crop + centre crop to 224 x 224) feeds the single-tile encoders "
                           f"{CLIP_RULE_ENCODERS} only; encoder = {encoder!r} has its own multi-tile preprocessing")
        return rule
    if rule not in RESIZE_RULES:
        raise MmeError(f"resize_rule = {resize_rule!r}; supported {RESIZE_RULES} (None means 'fit_pad'), 'checkpoint' (what the directory's "
                       "preprocessor_config.json asks for) and a ResizeSpec")
    if rule == "clip" and encoder not in CLIP_RULE_ENCODERS:
        raise MmeError(f"resize_rule = 'clip' (shortest-edge BICUBIC resize + centre crop to 224 x 224) feeds the single-tile encoders "
                       f"{CLIP_RULE_ENCODERS} only; encoder = {encoder!r} has its own multi-tile preprocessing")
    return rule


def _check_clip_rule_fields(pc: dict, where: str):
    """Under resize_rule = "clip" the file must describe exactly what the kernels do (CLIPImageProcessor's defaults)."""
    resample = pc.get("resample", 3)
    if resample != 3:
        raise MmeError(f"{where}: resample = {resample!r}; resize_rule = 'clip' resizes with Pillow BICUBIC (resample = 3) only")
    size = pc.get("size", {"shortest_edge": 224})
    if not (size == {"shortest_edge": 224} or (isinstance(size, int) and not isinstance(size, bool) and size == 224)):
        raise MmeError(f"{where}: size = {size!r}; resize_rule = 'clip' supports size = {{'shortest_edge': 224}} (or the bare int 224) only")
    if pc.get("do_resize", True) is False:
        raise MmeError(f"{where}: do_resize = False; resize_rule = 'clip' always resizes (supported: do_resize = True)")
    if pc.get("do_center_crop", True) is not True:
        raise MmeError(f"{where}: do_center_crop = {pc.get('do_center_crop')!r}; resize_rule = 'clip' always centre-crops (supported: do_center_crop = True)")
    crop = pc.get("crop_size", 224)
    if not (crop == {"height": 224, "width": 224} or (isinstance(crop, int) and not isinstance(crop, bool) and crop == 224)):
        raise MmeError(f"{where}: crop_size = {crop!r}; resize_rule = 'clip' supports crop_size = 224 x 224 ({{'height': 224, 'width': 224}} or 224) only")


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


SPEC_EDGES = (224, 512)  # mme_set_resize_spec: edge, height and width of the resized image


def resize_spec_of(preprocessor_config: dict, where: str = "preprocessor_config.json") -> ResizeSpec:
    """The ResizeSpec a preprocessor_config.json (the dict) asks for: what the Pillow backend of its image processor does
    before rescale and normalise -- resize the whole crop (`size`, `resample`), then `center_crop`.  Raises MmeError naming
    the field, its value and the supported set for everything K1 does not run.  `where` names the file in the messages."""
    pc = preprocessor_config
    kind = str(pc.get("image_processor_type", ""))
    if "Mllama" in kind or "max_image_tiles" in pc:
        raise MmeError(f"{where}: image_processor_type = {kind!r}; a Mllama processor tiles the image, which no resize spec describes: supported "
                       "encoder='mllama_tiles' (its own preprocessing) or the default fit-and-pad rule")
    if "max_num_patches" in pc:
        raise MmeError(f"{where}: max_num_patches = {pc['max_num_patches']!r}; a SigLIP 2 NaFlex processor keeps the aspect on a variable patch grid: "
                       "supported fixed-resolution processors only (size + resample, no max_num_patches)")
    if pc.get("do_resize", True) is False:
        raise MmeError(f"{where}: do_resize = False; a resize spec always resizes (supported: do_resize = True)")
    if pc.get("do_pad"):
        raise MmeError(f"{where}: do_pad = {pc['do_pad']!r}; supported: no padding (do_pad absent or False)")
    if pc.get("do_rescale", True) is not True:
        raise MmeError(f"{where}: do_rescale = {pc.get('do_rescale')!r}; K1 always rescales by 1/255 (supported: do_rescale = True)")
    rf = pc.get("rescale_factor", 1.0 / 255.0)
    if not isinstance(rf, (int, float)) or isinstance(rf, bool) or abs(float(rf) - 1.0 / 255.0) > 1e-9:
        raise MmeError(f"{where}: rescale_factor = {rf!r}; supported 1/255 = {1.0 / 255.0!r}")
    resample = pc.get("resample")
    if not _is_int(resample) or resample not in (2, 3):
        raise MmeError(f"{where}: resample = {resample!r}; supported 2 (Pillow BILINEAR) and 3 (Pillow BICUBIC)")
    size = pc.get("size")
    lo, hi = SPEC_EDGES
    if _is_int(size) or (isinstance(size, dict) and set(size) == {"shortest_edge"} and _is_int(size["shortest_edge"])):
        edge = size if _is_int(size) else size["shortest_edge"]
        mode, height, width = "shortest_edge", edge, 0
        ok = lo <= edge <= hi
    elif isinstance(size, dict) and set(size) == {"height", "width"} and _is_int(size["height"]) and _is_int(size["width"]):
        mode, height, width = "exact", size["height"], size["width"]
        ok = lo <= height <= hi and lo <= width <= hi
    else:
        ok = False
    if not ok:
        raise MmeError(f"{where}: size = {size!r}; supported {{'shortest_edge': S}}, the bare int S or {{'height': H, 'width': W}} with S, H, W in {lo}..{hi}")
    crop_on = pc.get("do_center_crop", False)
    if crop_on is True:
        crop = pc.get("crop_size")
        if not (crop == {"height": 224, "width": 224} or (_is_int(crop) and crop == 224)):
            raise MmeError(f"{where}: crop_size = {crop!r}; supported 224 x 224 ({{'height': 224, 'width': 224}} or 224)")
    elif crop_on not in (False, None):
        raise MmeError(f"{where}: do_center_crop = {crop_on!r}; supported True and False")
    elif mode == "shortest_edge":
        raise MmeError(f"{where}: do_center_crop = {pc.get('do_center_crop')!r} with size = {size!r}; a shortest-edge resize leaves no 224 x 224 image: "
                       "supported do_center_crop = True with crop_size 224 x 224")
    elif (height, width) != (224, 224):
        raise MmeError(f"{where}: do_center_crop = {pc.get('do_center_crop')!r} with size = {size!r}; without a centre crop the resized image is the "
                       "canvas: supported size 224 x 224, or do_center_crop = True with crop_size 224 x 224")
    return ResizeSpec(mode, height, width, resample)


def _read_preprocessor(path: str, encoder: str, resize_rule="fit_pad"):
    """preprocessor_config.json -> (mean, std, spec): mean / std or None / None; spec is the file's ResizeSpec under
    resize_rule = "checkpoint", else None.  Raises for what K1 cannot honour under `resize_rule`."""
    spec = resize_spec_of(_load_json(path), os.path.basename(path)) if resize_rule == "checkpoint" else None  # its refusals speak of the spec
    mean, std = _read_mean_std(path, encoder, resize_rule)
    return mean, std, spec


def _read_mean_std(path: str, encoder: str, resize_rule):
    global _warned_resize_rule
    pc = _load_json(path)
    where = os.path.basename(path)
    if pc.get("do_rescale", True) is not True:
        raise MmeError(f"{where}: do_rescale = {pc.get('do_rescale')!r}; K1 always rescales by 1/255")
    rf = pc.get("rescale_factor", 1.0 / 255.0)
    if abs(float(rf) - 1.0 / 255.0) > 1e-9:
        raise MmeError(f"{where}: rescale_factor = {rf!r}; K1 rescales by 1/255 = {1.0 / 255.0!r}")
    if pc.get("do_normalize", True) is not True:
        raise MmeError(f"{where}: do_normalize = {pc.get('do_normalize')!r}; K1 always normalises with image_mean / image_std")
    if resize_rule == "clip":
        _check_clip_rule_fields(pc, where)
        return _mean_std(pc, where)
    if resize_rule == "checkpoint" or isinstance(resize_rule, ResizeSpec):  # the caller's rule, not the fit-and-pad one: nothing to warn of
        return _mean_std(pc, where)
    resample = pc.get("resample", 2)
    clip_rule = encoder == "clip" and (resample == 3 or pc.get("do_center_crop") or "crop_size" in pc)
    if encoder == "dinov2":
        # DINOv2's processor (BitImageProcessor: shortest edge 256, BICUBIC, centre crop 224) is not a rule K1 has
        if resample != 2 or pc.get("do_center_crop") or "crop_size" in pc:
            named = [f"{k} = {pc[k]!r}" for k in ("image_processor_type", "resample", "size", "do_center_crop", "crop_size") if k in pc]
            logger.warning(f"{where}: {', '.join(named) or 'the file'} asks for DINOv2's own preprocessing, a shortest-edge-256 BICUBIC resize and a "
                           "224 x 224 centre crop; K1 does not run that rule by default: it keeps the aspect-preserving fit into 224 x 224 with zero padding "
                           "(resize_rule='checkpoint' runs the file's own rule, 'clip' CLIP's) and applies only the checkpoint's image_mean / image_std")
        return _mean_std(pc, where)
    if encoder == "siglip":
        # SiglipImageProcessor resizes to size x size WITHOUT keeping the aspect (any resample): not a rule K1 has
        if "Siglip" in str(pc.get("image_processor_type", "")) or resample != 2:
            named = [f"{k} = {pc[k]!r}" for k in ("image_processor_type", "resample", "size") if k in pc]
            logger.warning(f"{where}: {', '.join(named) or 'the file'} asks for SigLIP's own preprocessing, a plain resize to 224 x 224 that does not keep the "
                           "aspect ratio; K1 does not run that rule by default: it keeps the aspect-preserving fit into 224 x 224 with zero padding "
                           "(resize_rule='checkpoint' runs the file's own rule, 'clip' CLIP's) and applies only the checkpoint's image_mean / image_std")
        return _mean_std(pc, where)
    if resample != 2 and not (encoder == "clip" and resample == 3):
        raise MmeError(f"{where}: resample = {resample!r}; K1 resizes with Pillow BILINEAR (resample = 2) only")
    if encoder == "mllama_tiles":
        size = pc.get("size", {"height": 560, "width": 560})
        if not isinstance(size, dict) or size.get("height") != 560 or size.get("width") != 560:
            raise MmeError(f"{where}: size = {size!r}; the tile encoder is built for size = 560 x 560")
        tiles = pc.get("max_image_tiles", 4)
        if tiles != 4:
            raise MmeError(f"{where}: max_image_tiles = {tiles!r}; the tile encoder is built for max_image_tiles = 4")
    elif ("Mllama" not in str(pc.get("image_processor_type", "")) or clip_rule) and not _warned_resize_rule:
        _warned_resize_rule = True
        clip_fields = ""
        if clip_rule:  # CLIP's own rule: shortest edge to `size` with BICUBIC, then a centre crop
            named = [f"{k} = {pc[k]!r}" for k in ("resample", "size", "do_center_crop", "crop_size") if k in pc]
            clip_fields = f" ({', '.join(named)}: the shortest-edge BICUBIC resize and the centre crop are not applied)"
        logger.warning(f"{where}: image_processor_type = {pc.get('image_processor_type')!r} does not use Mllama's fit-and-pad resize{clip_fields}; K1 keeps the "
                       "aspect-preserving fit into 224 x 224 with zero padding (this encoder's contract, DESIGN.md) and applies only the "
                       "checkpoint's image_mean / image_std")
    return _mean_std(pc, where)


def _mean_std(pc: dict, where: str):
    mean, std = pc.get("image_mean"), pc.get("image_std")
    if mean is None or std is None:
        return None, None
    if len(mean) != 3 or len(std) != 3:
        raise MmeError(f"{where}: image_mean / image_std must have three channels, got {mean!r} / {std!r}")
    return tuple(float(v) for v in mean), tuple(float(v) for v in std)


# ---- tensors ------------------------------------------------------------------------------------------------------------
def _read_tensors(path: str, canonical, wanted: set):
    """-> ({canonical name: torch tensor}, {canonical name: key in the file}, [files read]); reads only the keys that map
    to a wanted name."""
    import torch

    single = os.path.join(path, "model.safetensors")
    index = os.path.join(path, "model.safetensors.index.json")
    legacy = os.path.join(path, "pytorch_model.bin")
    out, keys, files = {}, {}, []

    def take(name, key, tensor):
        if name in out:
            raise MmeError(f"{path}: the keys {keys[name]!r} and {key!r} both name the tensor {name!r}")
        out[name], keys[name] = tensor, key

    if os.path.exists(single) or os.path.exists(index):
        from safetensors import safe_open

        if os.path.exists(single):
            shards = {single: None}
        else:
            files.append(index)
            shards = {}
            for key, shard in _load_json(index)["weight_map"].items():
                if canonical(key) in wanted:
                    shards.setdefault(os.path.join(path, shard), []).append(key)
        for shard, shard_keys in shards.items():
            if not os.path.exists(shard):
                raise MmeError(f"{shard} is named by {os.path.basename(index)} and missing")
            files.append(shard)
            with safe_open(shard, framework="pt", device="cpu") as f:
                for key in (f.keys() if shard_keys is None else shard_keys):
                    name = canonical(key)
                    if name in wanted:
                        take(name, key, f.get_tensor(key))
    elif os.path.exists(legacy):
        files.append(legacy)
        try:
            sd = torch.load(legacy, map_location="cpu", weights_only=True, mmap=True)
        except (RuntimeError, ValueError):  # a file saved without the zip container cannot be mapped
            sd = torch.load(legacy, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        for key, tensor in sd.items():
            name = canonical(key)
            if name in wanted and isinstance(tensor, torch.Tensor):
                take(name, key, tensor)
    else:
        raise MmeError(f"{path}: no model.safetensors, model.safetensors.index.json or pytorch_model.bin")
    return out, keys, files


def _unify_dtype(tensors: dict, keys: dict):
    """All tensors in ONE of f32 / bf16 / f16: the dtype that holds most elements, when every other tensor converts to it
    exactly; else everything f32 (exact for all three)."""
    import torch

    names = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}
    count = {}
    for name, t in tensors.items():
        if t.dtype not in names:
            raise MmeError(f"tensor {keys[name]!r} has dtype {t.dtype}; supported: float32, bfloat16, float16")
        count[t.dtype] = count.get(t.dtype, 0) + t.numel()
    major = max(count, key=lambda d: count[d])
    if len(count) > 1 and major != torch.float32:
        for t in tensors.values():
            if t.dtype != major and not torch.equal(t.to(major).to(t.dtype), t):
                major = torch.float32
                break
    return {n: (t if t.dtype == major else t.to(major)).contiguous() for n, t in tensors.items()}, names[major]


# ---- what only some encoders need once the tensors are read (`encoders.Encoder.after_read`) ---------------------------------
def _optional_projection(name: str):
    """CLIP's two towers: a checkpoint without the projection `name` (CLIPVisionModel, CLIPTextModel) embeds with the final
    LayerNorm's row, whatever config.json says; one with it needs a projection_dim there."""
    def after_read(geometry, tensors, keys, path, where):
        if name not in tensors:
            return dataclasses.replace(geometry, projection_dim=None)
        if geometry.projection_dim is None:
            raise MmeError(f"{path}: the checkpoint holds {keys[name]!r} but {where} names no projection_dim")
        return geometry

    return after_read


def _dinov2_position_grid(geometry, tensors, keys, path, where):
    """The side of the position grid is the tensor's, not config.json's."""
    if DINOV2_POSITIONS not in tensors:
        return geometry
    rows = int(tensors[DINOV2_POSITIONS].shape[-2]) if tensors[DINOV2_POSITIONS].dim() >= 2 else 0
    grid = int(round(max(rows - 1, 0) ** 0.5))
    if rows < 2 or grid * grid != rows - 1:
        raise MmeError(f"{path}: tensor {keys[DINOV2_POSITIONS]!r} has shape {tuple(tensors[DINOV2_POSITIONS].shape)}: the patch part "
                       f"({rows - 1} rows) is no square grid")
    return dataclasses.replace(geometry, position_grid=grid)


def _siglip_logit_pair(geometry, tensors, keys, path, where):
    """A SiglipTextModel checkpoint has no logit_scale / logit_bias; a whole SiglipModel stores both as [1], kept beside the tower's tensors."""
    have = [k for k in SIGLIP_LOGIT_KEYS if k in tensors]
    if len(have) == 1:
        raise MmeError(f"{path}: the checkpoint holds {have[0]!r} without the other of {SIGLIP_LOGIT_KEYS}")
    for k in have:
        if tensors[k].numel() != 1:
            raise MmeError(f"{path}: tensor {keys[k]!r} has shape {tuple(tensors[k].shape)}, expected one value")
        tensors[k] = tensors[k].reshape(1)
    return geometry


def read_checkpoint(path, encoder: str = "vit_b16", resize_rule=None) -> Checkpoint:
    """Directory -> Checkpoint (see the module docstring).  Raises MmeError naming the file, field or key at fault.

    `resize_rule` ("fit_pad", the same as None, "clip", "checkpoint" or a ResizeSpec) is the rule K1 will run: under "clip" a
    preprocessor_config.json must describe CLIPImageProcessor's shortest-edge-224 BICUBIC resize and 224 x 224 centre crop
    exactly, and a directory without one gets CLIP's defaults (the engine's mean / std).  Under "checkpoint" the file must
    exist; `resize_spec_of` derives the rule from it (`Checkpoint.resize_spec`) before any tensor is read."""
    from .encoders import ENCODER_TABLE

    path = os.fspath(path)
    if encoder not in ENCODERS:
        raise ValueError(f"encoder must be one of {ENCODERS}")
    rec = ENCODER_TABLE[encoder]
    resize_rule = check_resize_rule(resize_rule, encoder)
    if not os.path.isdir(path):
        raise MmeError(f"{path!r} is not a local checkpoint directory; this engine never fetches")
    cfg_path = os.path.join(path, "config.json")
    if not os.path.exists(cfg_path):
        raise MmeError(f"{cfg_path} is missing")
    pre_path = os.path.join(path, "preprocessor_config.json")
    if resize_rule == "checkpoint":  # refused before anything is loaded
        if not os.path.exists(pre_path):
            raise MmeError(f"{pre_path} is missing: resize_rule = 'checkpoint' reads the rule from it (pass a ResizeSpec to name one yourself)")
        resize_spec_of(_load_json(pre_path), os.path.basename(pre_path))
    geometry, where = rec.config_geometry(_load_json(cfg_path), path)
    tensors, keys, files = _read_tensors(path, rec.canonical_name, {s[0] for s in rec.tensor_specs(geometry)} | set(rec.optional))
    if rec.after_read:  # what config.json cannot say: which optional tensors the file holds, the side of DINOv2's position grid
        geometry = rec.after_read(geometry, tensors, keys, path, where)
    specs = [(s[0], s[1]) for s in rec.tensor_specs(geometry)]
    specs += [(k, tuple(tensors[k].shape)) for k in rec.optional if k in tensors and k not in dict(specs)]
    for name, shape in specs:
        if name not in tensors:
            raise MmeError(f"{path}: tensor {name!r} is missing from the checkpoint")
        if tuple(tensors[name].shape) != tuple(shape):
            raise MmeError(f"{path}: tensor {keys[name]!r} has shape {tuple(tensors[name].shape)}, expected {tuple(shape)}")
    tensors, dtype = _unify_dtype({n: tensors[n] for n, _ in specs}, keys)
    mean = std = spec = None
    source = [cfg_path] + files
    if os.path.exists(pre_path) and not rec.text:  # a text tower reads no pixels
        mean, std, spec = _read_preprocessor(pre_path, encoder, resize_rule)
        source.append(pre_path)
    extra = rec.extra(tensors) if rec.extra else {}
    return Checkpoint(encoder=encoder, tensors=tensors, dtype=dtype, geometry=geometry, image_mean=mean, image_std=std, resize_spec=spec, source=source,
                      extra=extra)


# ---- config.json of a geometry (`encoders.Encoder.config_json`: geometry, dtype name, the weight dict -> dict) ----------------
def _vit_config(g, dtype, weights):
    return {"architectures": ["ViTModel"], "model_type": "vit", "image_size": g.image_size, "patch_size": g.patch_size, "num_channels": g.num_channels,
            "hidden_size": g.hidden_size, "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads,
            "intermediate_size": g.intermediate_size, "hidden_act": "gelu", "qkv_bias": True, "layer_norm_eps": g.layer_norm_eps, "dtype": dtype}


def _clip_config(g, dtype, weights):
    cfg = {"architectures": ["CLIPVisionModelWithProjection" if g.projection_dim else "CLIPVisionModel"], "model_type": "clip_vision_model",
           "image_size": g.image_size, "patch_size": g.patch_size, "num_channels": g.num_channels, "hidden_size": g.hidden_size,
           "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads, "intermediate_size": g.intermediate_size,
           "hidden_act": g.hidden_act, "layer_norm_eps": g.layer_norm_eps, "attention_dropout": 0.0, "dtype": dtype}
    if g.projection_dim:
        cfg["projection_dim"] = g.projection_dim
    return cfg


def _siglip_config(g, dtype, weights):
    cfg = {"architectures": ["SiglipVisionModel"], "model_type": "siglip_vision_model", "image_size": g.image_size, "patch_size": g.patch_size,
           "num_channels": g.num_channels, "hidden_size": g.hidden_size, "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads,
           "intermediate_size": g.intermediate_size, "hidden_act": g.hidden_act, "layer_norm_eps": g.layer_norm_eps, "attention_dropout": 0.0,
           "dtype": dtype}
    if g.vision_use_head is not True:
        cfg["vision_use_head"] = g.vision_use_head
    return cfg


def _dinov2_config(g, dtype, weights):
    import numpy as np

    rows = int(np.shape(weights[DINOV2_POSITIONS])[-2]) if DINOV2_POSITIONS in weights else g.position_rows
    ratio = g.intermediate_size / g.hidden_size
    return {"architectures": ["Dinov2Model"], "model_type": "dinov2", "image_size": g.patch_size * int(round((rows - 1) ** 0.5)),
            "patch_size": g.patch_size, "num_channels": g.num_channels, "hidden_size": g.hidden_size, "num_hidden_layers": g.num_layers,
            "num_attention_heads": g.num_heads, "mlp_ratio": int(ratio) if ratio == int(ratio) else ratio, "hidden_act": g.hidden_act,
            "layer_norm_eps": g.layer_norm_eps, "qkv_bias": True, "use_swiglu_ffn": g.use_swiglu_ffn, "layerscale_value": 1.0, "dtype": dtype}


def _clip_text_config(g, dtype, weights):
    cfg = {"architectures": ["CLIPTextModelWithProjection" if g.projection_dim else "CLIPTextModel"], "model_type": "clip_text_model",
           "vocab_size": g.vocab_size, "hidden_size": g.hidden_size, "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads,
           "intermediate_size": g.intermediate_size, "max_position_embeddings": g.max_position_embeddings, "hidden_act": g.hidden_act,
           "layer_norm_eps": g.layer_norm_eps, "attention_dropout": 0.0, "eos_token_id": g.eos_token_id, "dtype": dtype}
    if g.projection_dim:
        cfg["projection_dim"] = g.projection_dim
    return cfg


def _siglip_text_config(g, dtype, weights):
    return {"architectures": ["SiglipTextModel"], "model_type": "siglip_text_model", "vocab_size": g.vocab_size, "hidden_size": g.hidden_size,
            "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads, "intermediate_size": g.intermediate_size,
            "max_position_embeddings": g.max_position_embeddings, "hidden_act": g.hidden_act, "layer_norm_eps": g.layer_norm_eps,
            "attention_dropout": 0.0, "pad_token_id": g.pad_token_id, "projection_size": g.projection_size, "dtype": dtype}


def _tile_config(g, dtype, weights):
    return {"architectures": ["MllamaVisionModel"], "model_type": "mllama_vision_model", "image_size": g.image_size, "patch_size": g.patch_size,
            "num_channels": g.num_channels, "hidden_size": g.hidden_size, "attention_heads": g.num_heads, "intermediate_size": g.intermediate_size,
            "hidden_act": "gelu", "max_num_tiles": g.max_num_tiles, "supported_aspect_ratios": SUPPORTED_ASPECT_RATIOS,
            "num_hidden_layers": g.num_layers, "num_global_layers": g.num_global_layers,
            "intermediate_layers_indices": list(g.intermediate_layers), "norm_eps": g.norm_eps, "dtype": dtype}


def _mllama_lm_config(g, dtype, weights):
    rope = {"rope_type": g.rope_type, "rope_theta": g.rope_theta}
    if g.rope_type == "llama3":
        rope.update({"factor": g.rope_factor, "low_freq_factor": g.rope_low_freq_factor, "high_freq_factor": g.rope_high_freq_factor,
                     "original_max_position_embeddings": g.rope_original_max})
    return {"architectures": ["MllamaForConditionalGeneration"], "model_type": "mllama", "image_token_index": g.image_token_id, "dtype": dtype,
            "text_config": {"model_type": "mllama_text_model", "hidden_size": g.hidden_size, "num_attention_heads": g.num_heads,
                            "num_key_value_heads": g.num_kv_heads, "intermediate_size": g.intermediate_size, "num_hidden_layers": g.num_layers,
                            "cross_attention_layers": list(g.cross_layers), "vocab_size": g.vocab_size, "rms_norm_eps": g.rms_norm_eps,
                            "hidden_act": g.hidden_act, "rope_parameters": rope},
            "vision_config": {"vision_output_dim": g.vision_output_dim}}


def save_checkpoint(path, weights: dict, encoder: str = "vit_b16", dtype: str = "float32", geometry=None, image_mean=None, image_std=None,
                    image_processor_type: str = "MllamaImageProcessor") -> str:
    """The inverse of `read_checkpoint` for a canonical-name dict of f32 arrays (weights.make_vit_weights /
    make_tile_vit_weights): writes config.json + model.safetensors in `dtype` (and preprocessor_config.json when a mean /
    std is given) into `path`.  What the tests and tools/bench_load.py load from; also how seeded weights become a
    directory another tool can read."""
    import numpy as np
    import torch
    from safetensors.torch import save_file

    from .encoders import ENCODER_TABLE

    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    os.makedirs(path, exist_ok=True)
    if encoder not in ENCODER_TABLE:
        raise ValueError(f"encoder must be one of {ENCODERS}")
    rec = ENCODER_TABLE[encoder]
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(rec.config_json(geometry or rec.geometry, dtype, weights), f, indent=1)
    save_file({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(tdt).contiguous() for k, v in weights.items()},
              os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
    if image_mean is not None:
        pc = {"image_processor_type": image_processor_type, "do_rescale": True, "rescale_factor": 1.0 / 255.0, "do_normalize": True, "resample": 2,
              "image_mean": [float(v) for v in image_mean], "image_std": [float(v) for v in image_std]}
        if encoder == "mllama_tiles":
            pc.update({"size": {"height": 560, "width": 560}, "max_image_tiles": 4})
        with open(os.path.join(path, "preprocessor_config.json"), "w", encoding="utf-8") as f:
            json.dump(pc, f, indent=1)
    return os.fspath(path)


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="python -m multimodal_embeddings_amd.checkpoint", description="what a load of this checkpoint directory would find")
    ap.add_argument("directory")
    ap.add_argument("--encoder", choices=CLI_ENCODERS, default="vit_b16")
    ap.add_argument("--resize-rule", choices=RESIZE_RULES + ("checkpoint",), default="fit_pad",
                    help="the rule K1 would run: 'clip' checks preprocessor_config.json against the shortest-edge BICUBIC resize + centre crop; "
                         "'checkpoint' derives the rule from that file and prints it")
    a = ap.parse_args(argv)
    try:
        ck = read_checkpoint(a.directory, "siglip" if a.encoder == SIGLIP_ALIAS else a.encoder, a.resize_rule)
    except MmeError as e:
        print(f"cannot load: {e}")
        return 1
    print(f"encoder     {ck.encoder}")
    print(f"dtype       {ck.dtype}")
    print(f"geometry    {ck.geometry}")
    print(f"image_mean  {ck.image_mean}")
    print(f"image_std   {ck.image_std}")
    if ck.resize_spec is not None:
        print(f"resize_spec {ck.resize_spec}")
    print(f"tensors     {len(ck.tensors)}")
    print(f"bytes       {ck.nbytes}")
    for f in ck.source:
        print(f"read        {f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
