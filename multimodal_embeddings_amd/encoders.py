"""One record per encoder kind: what differs between the towers, stated once.

`checkpoint.read_checkpoint` / `save_checkpoint`, `Engine._weights_struct` / `_load` / `_load_checkpoint` and RegionEmbedder look
an encoder up in ENCODER_TABLE (keyed by `checkpoint.ENCODERS`) and run one shared sequence; a new tower is a new record, its
`*_tensor_specs` / `make_*_weights` / `infer_*_geometry` in weights.py, its `config.json` pair in checkpoint.py and its struct in
_lib.py.  The tile tower has another layer record and scalar gates: it keeps its own builder and loaders and is here for dispatch.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Callable

from . import _lib, checkpoint as ck, weights as wt


@dataclass(frozen=True)
class Encoder:
    geometry: object                 # the default geometry; its class is the encoder's geometry class
    tensor_specs: Callable           # geometry -> [(name, shape, kind, ...)] in the fixed order
    make_weights: Callable           # (seed, geometry) -> seeded weight dict
    canonical_name: Callable         # checkpoint key -> name of tensor_specs | None
    config_geometry: Callable        # (config.json dict, directory) -> (geometry, where its fields were found); refuses what is not run
    config_json: Callable            # (geometry, dtype name, weight dict) -> config.json dict
    struct: type                     # the ctypes struct of include/mme.h
    symbol: str                      # "mme_load_X": the host load; symbol + "_as" prepares on the device
    infer_geometry: Callable | None = None  # weight dict -> geometry; None: the geometry is fixed or the caller's
    layer_prefix: str = ""           # "...{}.": a format over the layer index, in front of every name of `block`
    block: tuple | None = None       # the spelling of LAYER_FIELDS (+ DINOv2's two LayerScale names); None: the tile tower's own record
    top: dict = dataclasses.field(default_factory=dict)  # struct field -> tensor name outside the layers, None where the model has none
    scalars: Callable | None = None  # (struct, geometry, **special) fills the numbers, refusing what the struct cannot say
    fill: Callable | None = None     # (struct, geometry, arr): SigLIP's pooling head
    text: bool = False               # a text tower reads no preprocessor_config.json and loads beside the image tower
    optional: tuple = ()             # tensors a checkpoint may lack: CLIP's projections, SigLIP's logit_scale / logit_bias pair
    after_read: Callable | None = None      # (geometry, tensors, keys, directory, where) -> geometry, once the tensors are read
    extra: Callable | None = None    # tensors -> Checkpoint.extra
    host_geometry: Callable | None = None   # (weight dict, geometry | None) -> geometry of a host load, where inferring is not enough
    special: Callable | None = None  # (get(name), Checkpoint.extra | None) -> (special arguments of the builder, what to keep alive)
    library_refuses_depth: bool = False     # a layer count outside 1..64 skips the host's tensor checks: the library names it
    seed_offset: int = 0             # RegionEmbedder draws the tile tower at seed + 1
    beside: Callable | None = None   # text towers: embed_dim of the image side -> the seeded tower that embeds into it

    @property
    def geometry_class(self) -> type:
        return type(self.geometry)

    @property
    def loader(self) -> str:
        """The Engine method of the host load; + "_checkpoint": of the device load."""
        return self.symbol[len("mme_"):]

    def layer_names(self, i: int) -> dict:
        """Field of _lib._Layer (DINOv2: and of _Dinov2Scale) -> tensor name, for layer i."""
        prefix = self.layer_prefix.format(i)
        return dict(zip(wt.LAYER_FIELDS + ("lambda1", "lambda2"), (prefix + name for name in self.block)))


_VIT_TOP = {"cls_token": "embeddings.cls_token", "pos_emb": "embeddings.position_embeddings", "patch_w": "embeddings.patch_embeddings.projection.weight",
            "patch_b": "embeddings.patch_embeddings.projection.bias", "lnf_g": "layernorm.weight", "lnf_b": "layernorm.bias"}
_V, _T = "vision_model.", "text_model."
_TEXT_TOP = {"token_emb": _T + "embeddings.token_embedding.weight", "pos_emb": _T + "embeddings.position_embedding.weight",
             "lnf_g": _T + "final_layer_norm.weight", "lnf_b": _T + "final_layer_norm.bias"}


def _siglip_text_beside(D: int):
    b = wt.SIGLIP_TEXT_B
    return b if D == b.hidden_size else dataclasses.replace(b, hidden_size=D, num_heads=D // 64, intermediate_size=4 * D, projection_size=D)


_VIT = Encoder(
    geometry=wt.VIT_B16, tensor_specs=wt.vit_tensor_specs, make_weights=wt.make_vit_weights, infer_geometry=wt.infer_vit_geometry,
    canonical_name=ck.canonical_vit_name, config_geometry=ck._vit_family_geometry, config_json=ck._vit_config, struct=_lib._Weights,
    symbol="mme_load_vit", layer_prefix="layers.{}.", block=wt.VIT_BLOCK, top=_VIT_TOP, scalars=_lib._vit_scalars)

ENCODER_TABLE = {
    # exactly ViT-B/16: config.json must say so, and no other geometry is read off a weight dict
    "vit_b16": dataclasses.replace(_VIT, config_geometry=ck._vit_geometry, infer_geometry=None),
    "vit": _VIT,
    "clip": Encoder(
        geometry=wt.CLIP_B16, tensor_specs=wt.clip_tensor_specs, make_weights=wt.make_clip_weights, infer_geometry=wt.infer_clip_geometry,
        canonical_name=ck.canonical_clip_name, config_geometry=ck._clip_geometry, config_json=ck._clip_config, struct=_lib._ClipWeights,
        symbol="mme_load_clip", layer_prefix=_V + "encoder.layers.{}.", block=wt.CLIP_BLOCK, scalars=_lib._clip_scalars,
        top={"cls_token": _V + "embeddings.class_embedding", "pos_emb": _V + "embeddings.position_embedding.weight",
             "patch_w": _V + "embeddings.patch_embedding.weight", "patch_b": None,  # CLIPVisionEmbeddings: bias=False
             "lnf_g": _V + "post_layernorm.weight", "lnf_b": _V + "post_layernorm.bias", "pre_g": _V + "pre_layrnorm.weight",
             "pre_b": _V + "pre_layrnorm.bias", "proj_w": "visual_projection.weight"},
        optional=("visual_projection.weight",), after_read=ck._optional_projection("visual_projection.weight")),
    "mllama_tiles": Encoder(
        geometry=wt.TILE_VIT, tensor_specs=wt.tile_vit_tensor_specs, make_weights=wt.make_tile_vit_weights, canonical_name=ck.canonical_tile_name,
        config_geometry=ck._tile_geometry, config_json=ck._tile_config, struct=_lib._TileWeights, symbol="mme_load_tile_vit", seed_offset=1),
    "clip_text": Encoder(
        geometry=wt.CLIP_TEXT_B, tensor_specs=wt.clip_text_tensor_specs, make_weights=wt.make_clip_text_weights,
        infer_geometry=wt.infer_clip_text_geometry, canonical_name=ck.canonical_clip_text_name, config_geometry=ck._clip_text_geometry,
        config_json=ck._clip_text_config, struct=_lib._ClipTextWeights, symbol="mme_load_clip_text", layer_prefix=_T + "encoder.layers.{}.",
        block=wt.CLIP_BLOCK, top={**_TEXT_TOP, "proj_w": "text_projection.weight"}, scalars=_lib._clip_text_scalars, text=True,
        optional=("text_projection.weight",), after_read=ck._optional_projection("text_projection.weight"),
        beside=lambda D: dataclasses.replace(wt.CLIP_TEXT_B, projection_dim=D)),
    "siglip": Encoder(
        geometry=wt.SIGLIP_B16, tensor_specs=wt.siglip_tensor_specs, make_weights=wt.make_siglip_weights, infer_geometry=wt.infer_siglip_geometry,
        canonical_name=ck.canonical_siglip_name, config_geometry=ck._siglip_geometry, config_json=ck._siglip_config, struct=_lib._SiglipWeights,
        symbol="mme_load_siglip", layer_prefix=_V + "encoder.layers.{}.", block=wt.CLIP_BLOCK, scalars=_lib._siglip_scalars, fill=_lib._siglip_head,
        top={"cls_token": None,  # SiglipVisionEmbeddings: no class token
             "pos_emb": _V + "embeddings.position_embedding.weight", "patch_w": _V + "embeddings.patch_embedding.weight",
             "patch_b": _V + "embeddings.patch_embedding.bias", "lnf_g": _V + "post_layernorm.weight", "lnf_b": _V + "post_layernorm.bias",
             "probe": _V + "head.probe"}),
    "siglip_text": Encoder(
        geometry=wt.SIGLIP_TEXT_B, tensor_specs=wt.siglip_text_tensor_specs, make_weights=wt.make_siglip_text_weights,
        infer_geometry=wt.infer_siglip_text_geometry, canonical_name=ck.canonical_siglip_text_name, config_geometry=ck._siglip_text_geometry,
        config_json=ck._siglip_text_config, struct=_lib._SiglipTextWeights, symbol="mme_load_siglip_text", layer_prefix=_T + "encoder.layers.{}.",
        block=wt.CLIP_BLOCK, top={**_TEXT_TOP, "head_w": _T + "head.weight", "head_b": _T + "head.bias"}, scalars=_lib._siglip_text_scalars,
        text=True, optional=wt.SIGLIP_LOGIT_KEYS, after_read=ck._siglip_logit_pair, special=_lib._siglip_text_special,
        library_refuses_depth=True, beside=_siglip_text_beside),
    "dinov2": Encoder(
        geometry=wt.DINOV2_B14, tensor_specs=wt.dinov2_tensor_specs, make_weights=wt.make_dinov2_weights, infer_geometry=wt.infer_dinov2_geometry,
        canonical_name=ck.canonical_dinov2_name, config_geometry=ck._dinov2_geometry, config_json=ck._dinov2_config, struct=_lib._Dinov2Weights,
        symbol="mme_load_dinov2", layer_prefix="encoder.layer.{}.", block=wt.DINOV2_BLOCK + ("layer_scale1.lambda1", "layer_scale2.lambda1"),
        top=_VIT_TOP, scalars=_lib._dinov2_scalars, after_read=ck._dinov2_position_grid,
        extra=lambda tensors: {"position_table": ck.interpolate_dinov2_positions(tensors[ck.DINOV2_POSITIONS])},
        host_geometry=_lib._dinov2_host_geometry, special=_lib._dinov2_special, library_refuses_depth=True),
    # the Mllama language tower and projector: its own builder (Engine._mllama_lm_struct), as the tile tower; beside that tower in one directory
    "mllama_text": Encoder(
        geometry=wt.MLLAMA_LM_11B, tensor_specs=wt.mllama_lm_tensor_specs, make_weights=wt.make_mllama_lm_weights,
        infer_geometry=wt.infer_mllama_lm_geometry, canonical_name=ck.canonical_mllama_lm_name, config_geometry=ck._mllama_lm_geometry,
        config_json=ck._mllama_lm_config, struct=_lib._MllamaLMWeights, symbol="mme_load_mllama_lm", text=True, special=_lib._mllama_lm_special,
        seed_offset=6),
}
assert tuple(ENCODER_TABLE) == ck.ENCODERS
