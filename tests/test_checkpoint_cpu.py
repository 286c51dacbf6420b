"""Checkpoint reader (multimodal_embeddings_amd/checkpoint.py): names, dtypes, shards, configuration checks and the
`model_name` decision of RegionEmbedder -- host only, no GPU.  Seed 7 everywhere: not a default seed of the package."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd._lib import MmeError
from multimodal_embeddings_amd.weights import (TileViTGeometry, f32_to_bf16_bits, make_tile_vit_weights, make_vit_weights,
                                               tile_vit_tensor_specs, vit_tensor_specs)

SEED = 7
SHALLOW = TileViTGeometry(num_layers=2, num_global_layers=1, intermediate_layers=(0,))


@pytest.fixture(scope="module")
def vit_w():
    return make_vit_weights(SEED)


@pytest.fixture(scope="module")
def tile_w():
    return make_tile_vit_weights(SEED, SHALLOW)


def _bits(t: torch.Tensor) -> np.ndarray:
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _assert_equals_dict(ck, w, dtype):
    assert ck.dtype == dtype
    assert set(ck.tensors) == set(w)
    for name, want in w.items():
        got = ck.tensors[name]
        assert got.is_contiguous() and tuple(got.shape) == want.shape, name
        if dtype == "float32":
            assert np.array_equal(_bits(got), want.view(np.int32)), name
        else:
            assert dtype == "bfloat16"
            assert np.array_equal(_bits(got).view(np.uint16), f32_to_bf16_bits(want).reshape(want.shape)), name


# ---- 1. what transformers writes ----------------------------------------------------------------------------------------
def test_vit_model_save_pretrained_roundtrip(tmp_path, vit_w):
    transformers = pytest.importorskip("transformers")
    model = transformers.ViTModel(transformers.ViTConfig(), add_pooling_layer=False)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in vit_w.items()}, strict=True)
    model.save_pretrained(tmp_path)
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    assert list(ck.tensors) == [n for n, _, _ in vit_tensor_specs()]
    _assert_equals_dict(ck, vit_w, "float32")
    assert ck.geometry.layer_norm_eps == 1e-12 and ck.image_mean is None
    assert any(f.endswith("model.safetensors") for f in ck.source)


def test_vit_for_image_classification_prefix_and_classifier(tmp_path, vit_w):
    transformers = pytest.importorskip("transformers")
    model = transformers.ViTForImageClassification(transformers.ViTConfig(num_labels=3))
    model.vit.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in vit_w.items()}, strict=True)
    model.save_pretrained(tmp_path)
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    assert list(ck.tensors) == [n for n, _, _ in vit_tensor_specs()]
    _assert_equals_dict(ck, vit_w, "float32")


# ---- 2. hand-written directories ----------------------------------------------------------------------------------------
def _bf16_dict(w):
    return {k: torch.from_numpy(v.copy()).to(torch.bfloat16) for k, v in w.items()}


def test_canonical_bf16_safetensors(tmp_path, vit_w):
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16")
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    _assert_equals_dict(ck, vit_w, "bfloat16")
    assert ck.nbytes == sum(v.size for v in vit_w.values()) * 2


def test_two_shards_with_index(tmp_path, vit_w):
    from safetensors.torch import save_file

    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16")
    os.remove(tmp_path / "model.safetensors")
    sd = _bf16_dict(vit_w)
    names = sorted(sd)
    parts = {"model-00001-of-00002.safetensors": names[: len(names) // 2], "model-00002-of-00002.safetensors": names[len(names) // 2:]}
    weight_map = {}
    for fname, keys in parts.items():
        save_file({k: sd[k] for k in keys}, str(tmp_path / fname), metadata={"format": "pt"})
        weight_map.update({k: fname for k in keys})
    # a shard that holds nothing the encoder needs is never opened: it does not even exist
    weight_map["classifier.weight"] = "model-00003-of-00003.safetensors"
    (tmp_path / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": weight_map}))
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    _assert_equals_dict(ck, vit_w, "bfloat16")
    assert sum(f.endswith(".safetensors") for f in ck.source) == 2


def test_pytorch_model_bin(tmp_path, vit_w):
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16")
    os.remove(tmp_path / "model.safetensors")
    torch.save(_bf16_dict(vit_w), tmp_path / "pytorch_model.bin")
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    _assert_equals_dict(ck, vit_w, "bfloat16")


def test_minority_dtype_follows_the_majority_when_exact(tmp_path, vit_w):
    from safetensors.torch import save_file

    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16")
    sd = _bf16_dict(vit_w)
    sd["layernorm.bias"] = torch.from_numpy(vit_w["layernorm.bias"].copy())  # f32, bf16-representable values
    save_file(sd, str(tmp_path / "model.safetensors"))
    _assert_equals_dict(ckpt.read_checkpoint(tmp_path, "vit_b16"), vit_w, "bfloat16")
    inexact = vit_w["layernorm.bias"].copy()
    inexact[0] = np.float32(1.0 + 2.0 ** -20)
    sd["layernorm.bias"] = torch.from_numpy(inexact)
    save_file(sd, str(tmp_path / "model.safetensors"))
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    assert ck.dtype == "float32" and all(t.dtype == torch.float32 for t in ck.tensors.values())
    assert ck.tensors["layernorm.bias"][0].item() == float(inexact[0])
    assert np.array_equal(ck.tensors["layers.3.mlp.fc1.weight"].numpy(), vit_w["layers.3.mlp.fc1.weight"])


# ---- 3. Mllama vision tower ---------------------------------------------------------------------------------------------
def test_mllama_vision_model_saved_and_nested(tmp_path, tile_w):
    pytest.importorskip("transformers")
    from safetensors import safe_open
    from safetensors.torch import save_file
    from transformers.models.mllama.configuration_mllama import MllamaVisionConfig
    from transformers.models.mllama.modeling_mllama import MllamaVisionModel

    cfg = MllamaVisionConfig(image_size=560, num_hidden_layers=2, num_global_layers=1, intermediate_layers_indices=[0])
    model = MllamaVisionModel(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in tile_w.items()}, strict=True)
    model = model.to(torch.bfloat16)
    plain = tmp_path / "plain"
    model.save_pretrained(plain)
    ck = ckpt.read_checkpoint(plain, "mllama_tiles")
    assert ck.geometry == SHALLOW
    assert list(ck.tensors) == [n for n, _, _, _ in tile_vit_tensor_specs(SHALLOW)]
    _assert_equals_dict(ck, tile_w, "bfloat16")

    nested = tmp_path / "nested"
    nested.mkdir()
    with safe_open(str(plain / "model.safetensors"), framework="pt") as f:
        sd = {"model.vision_model." + k: f.get_tensor(k) for k in f.keys()}
    sd["model.language_model.layers.0.self_attn.q_proj.weight"] = torch.zeros(8, 8, dtype=torch.float64)  # never read: f64 would be refused
    save_file(sd, str(nested / "model.safetensors"), metadata={"format": "pt"})
    vision_cfg = json.loads((plain / "config.json").read_text())
    (nested / "config.json").write_text(json.dumps({"model_type": "mllama", "vision_config": vision_cfg, "text_config": {"hidden_size": 4096}}))
    ck2 = ckpt.read_checkpoint(nested, "mllama_tiles")
    assert ck2.geometry == SHALLOW
    _assert_equals_dict(ck2, tile_w, "bfloat16")


def test_save_checkpoint_tile_roundtrip(tmp_path, tile_w):
    ckpt.save_checkpoint(tmp_path, tile_w, "mllama_tiles", "bfloat16", SHALLOW, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5))
    ck = ckpt.read_checkpoint(tmp_path, "mllama_tiles")
    assert ck.geometry == SHALLOW and ck.image_mean == (0.5, 0.5, 0.5) and ck.image_std == (0.5, 0.5, 0.5)
    _assert_equals_dict(ck, tile_w, "bfloat16")


# ---- 4. errors name their cause -----------------------------------------------------------------------------------------
@pytest.fixture()
def vit_dir(tmp_path, vit_w):
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16", image_mean=(0.5, 0.5, 0.5), image_std=(0.25, 0.5, 0.75))
    return tmp_path


def _edit_json(path, **changes):
    d = json.loads(path.read_text())
    d.update(changes)
    path.write_text(json.dumps(d))


def test_preprocessor_mean_std_are_returned(vit_dir):
    ck = ckpt.read_checkpoint(vit_dir, "vit_b16")
    assert ck.image_mean == (0.5, 0.5, 0.5) and ck.image_std == (0.25, 0.5, 0.75)
    assert str(vit_dir / "preprocessor_config.json") in ck.source


def test_missing_key_is_named(vit_dir, vit_w):
    from safetensors.torch import save_file

    sd = _bf16_dict(vit_w)
    del sd["layers.5.mlp.fc2.bias"]
    save_file(sd, str(vit_dir / "model.safetensors"))
    with pytest.raises(MmeError, match=r"layers\.5\.mlp\.fc2\.bias"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_wrong_shape_is_named(vit_dir, vit_w):
    from safetensors.torch import save_file

    sd = _bf16_dict(vit_w)
    sd["layers.2.attention.k_proj.bias"] = sd["layers.2.attention.k_proj.bias"][:700].contiguous()
    save_file(sd, str(vit_dir / "model.safetensors"))
    with pytest.raises(MmeError, match=r"layers\.2\.attention\.k_proj\.bias.*700.*768"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_hidden_size_mismatch_names_field_found_and_built(vit_dir):
    _edit_json(vit_dir / "config.json", hidden_size=1024)
    with pytest.raises(MmeError, match=r"hidden_size = 1024.*built for hidden_size = 768"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_rescale_factor_is_refused(vit_dir):
    _edit_json(vit_dir / "preprocessor_config.json", rescale_factor=1.0 / 127.5)
    with pytest.raises(MmeError, match="rescale_factor"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_resample_is_refused(vit_dir):
    _edit_json(vit_dir / "preprocessor_config.json", resample=3)
    with pytest.raises(MmeError, match="resample = 3"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_do_normalize_false_and_do_rescale_false_are_refused(vit_dir):
    _edit_json(vit_dir / "preprocessor_config.json", do_normalize=False)
    with pytest.raises(MmeError, match="do_normalize"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")
    _edit_json(vit_dir / "preprocessor_config.json", do_normalize=True, do_rescale=False)
    with pytest.raises(MmeError, match="do_rescale"):
        ckpt.read_checkpoint(vit_dir, "vit_b16")


def test_tile_processor_size_and_tiles(tmp_path, tile_w):
    ckpt.save_checkpoint(tmp_path, tile_w, "mllama_tiles", "bfloat16", SHALLOW, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5))
    _edit_json(tmp_path / "preprocessor_config.json", max_image_tiles=2)
    with pytest.raises(MmeError, match="max_image_tiles = 2"):
        ckpt.read_checkpoint(tmp_path, "mllama_tiles")
    _edit_json(tmp_path / "preprocessor_config.json", max_image_tiles=4, size={"height": 448, "width": 448})
    with pytest.raises(MmeError, match="size"):
        ckpt.read_checkpoint(tmp_path, "mllama_tiles")


def test_vit_image_processor_is_a_warning_not_an_error(vit_dir, caplog):
    _edit_json(vit_dir / "preprocessor_config.json", image_processor_type="ViTImageProcessor", size={"height": 224, "width": 224})
    ckpt._warned_resize_rule = False
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(vit_dir, "vit_b16")
        ckpt.read_checkpoint(vit_dir, "vit_b16")
    assert ck.image_mean == (0.5, 0.5, 0.5)
    hits = [r for r in caplog.records if "aspect-preserving fit" in r.getMessage()]
    assert len(hits) == 1 and hits[0].levelno == logging.WARNING


def test_model_name_decision(tmp_path, caplog):
    assert ckpt.resolve_model_source("anything", weights={"x": 1}) == "weights"
    assert ckpt.resolve_model_source(str(tmp_path)) == "checkpoint"
    assert ckpt.resolve_model_source(tmp_path, allow_synthetic=False) == "checkpoint"
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        assert ckpt.resolve_model_source("intfloat/mmE5-mllama-11b-instruct") == "synthetic"
    assert any("SYNTHETIC" in r.getMessage() for r in caplog.records)
    with pytest.raises(MmeError, match="not a local checkpoint directory; this engine never fetches"):
        ckpt.resolve_model_source("intfloat/mmE5-mllama-11b-instruct", allow_synthetic=False)
    with pytest.raises(MmeError, match="never fetches"):
        ckpt.read_checkpoint(str(tmp_path / "absent"), "vit_b16")


def test_region_embedder_refuses_a_name_before_touching_a_device():
    """allow_synthetic=False with a name that is no directory: MmeError from the constructor, on a machine with or without a GPU."""
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(MmeError, match="not a local checkpoint directory; this engine never fetches"):
        RegionEmbedder("intfloat/mmE5-mllama-11b-instruct", device=0, allow_synthetic=False)


def test_command_line_report(vit_dir, capsys):
    assert ckpt.main([str(vit_dir)]) == 0
    out = capsys.readouterr().out
    assert "bfloat16" in out and "tensors     198" in out and "image_mean  (0.5, 0.5, 0.5)" in out
    _edit_json(vit_dir / "config.json", hidden_size=1024)
    assert ckpt.main([str(vit_dir)]) == 1
    assert "hidden_size = 1024" in capsys.readouterr().out
