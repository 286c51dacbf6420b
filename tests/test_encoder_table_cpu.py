"""encoders.ENCODER_TABLE: one record per encoder kind, and each record agrees with itself.

The builder must ask for exactly the tensors the record's `tensor_specs` lists, and `infer_geometry` must read back the geometry
`make_weights` was called with.  No GPU and no library load: `Engine._weights_struct` is given an `arr` that only records."""
import dataclasses

import pytest

from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd._lib import Engine
from multimodal_embeddings_amd.encoders import ENCODER_TABLE
from multimodal_embeddings_amd.weights import LAYER_FIELDS, TileViTGeometry

R = dataclasses.replace


def two_layers(kind, **change):
    """The record's default geometry cut to 2 layers (the tile tower: 2 local + 1 global), text vocabularies cut to 64 ids."""
    rec = ENCODER_TABLE[kind]
    if kind == "mllama_tiles":
        return TileViTGeometry(num_layers=2, num_global_layers=1, intermediate_layers=(0,))
    if kind == "clip_text":
        change = {"vocab_size": 64, "eos_token_id": 63, **change}
    if kind == "siglip_text":
        change = {"vocab_size": 64, **change}
    return R(rec.geometry, num_layers=2, **change)


def width(D):
    return dict(hidden_size=D, num_heads=D // 64, intermediate_size=4 * D)


def asked(kind, geom):
    """[(name, first element)] in the order the builder asks for them; the tile tower's gates as (name, "gate")."""
    calls = []

    def arr(name, first=0):
        calls.append((name, first))

    def gate(name):
        calls.append((name, "gate"))
        return 0.0

    Engine._weights_struct(kind, geom, arr, **({"gate": gate} if kind == "mllama_tiles" else {}))
    return calls


def test_every_encoder_has_a_record():
    assert tuple(ENCODER_TABLE) == ckpt.ENCODERS
    for kind, rec in ENCODER_TABLE.items():
        assert isinstance(rec.geometry, rec.geometry_class) and rec.symbol.startswith("mme_load_") and hasattr(Engine, rec.loader), kind
        assert hasattr(Engine, rec.loader + "_checkpoint"), kind
        assert rec.text == kind.endswith("_text"), kind
    b16, vit = ENCODER_TABLE["vit_b16"], ENCODER_TABLE["vit"]  # they differ in how config.json becomes a geometry, and in nothing else a load uses
    assert b16.infer_geometry is None and R(b16, config_geometry=vit.config_geometry, infer_geometry=vit.infer_geometry) == vit


@pytest.mark.parametrize("kind", ckpt.ENCODERS)
def test_builder_asks_for_the_names_of_the_specs(kind):
    rec, geom = ENCODER_TABLE[kind], two_layers(kind)
    names = [s[0] for s in rec.tensor_specs(geom)]
    calls = asked(kind, geom)
    assert len(set(names)) == len(names) and {n for n, _ in calls} == set(names)
    split = {n for n, first in calls if first not in (0, "gate")}  # SigLIP's in_proj pair: asked for at three element offsets
    assert split == ({"vision_model.head.attention.in_proj_weight", "vision_model.head.attention.in_proj_bias"} if kind == "siglip" else set())
    assert len(calls) == len(names) + 2 * len(split)
    if rec.block is not None:
        for i in range(2):
            layer = rec.layer_names(i)
            assert tuple(layer)[:16] == LAYER_FIELDS and set(layer.values()) <= set(names)
        assert f"{rec.layer_prefix.format(2)}{rec.block[0]}" not in names
    # the documented optional tensors: CLIP's projections are asked for only by a geometry that has one; SigLIP's two logit scalars
    # travel as numbers, never as pointers
    for name in rec.optional:
        if "projection" in name:
            assert name in names and name not in {n for n, _ in asked(kind, R(geom, projection_dim=None))}
        else:
            assert name not in names


@pytest.mark.parametrize("kind,change", [("vit", {}), ("vit", width(384)), ("vit", {"patch_size": 32}), ("clip", {}), ("clip", width(384)),
                                         ("clip", {"projection_dim": None}), ("siglip", {}), ("siglip", width(384)), ("dinov2", {}),
                                         ("dinov2", {**width(384), "position_grid": 37}), ("clip_text", {}), ("clip_text", {**width(768), "projection_dim": None}),
                                         ("siglip_text", {}), ("siglip_text", {**width(512), "projection_size": 256})])
def test_infer_geometry_reads_back_what_make_weights_was_given(kind, change):
    rec, geom = ENCODER_TABLE[kind], two_layers(kind, **change)
    w = rec.make_weights(1, geom)
    assert list(w)[: len(rec.tensor_specs(geom))] == [s[0] for s in rec.tensor_specs(geom)]
    # every field is either in the shapes or at the default the geometry was derived from (eps, the activation, the token ids)
    assert rec.infer_geometry(w) == geom
