"""The ViT/16 family on the host: the "vit" encoder name of checkpoint.py (geometry read from config.json and checked
against the supported set), the geometry presets and the FLOP count of weights.py.  No GPU.  Seed 7, as the other
checkpoint tests; shallow (2- and 3-layer) ViT-S and ViT-L variants keep the tensors small."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd._lib import MmeError
from multimodal_embeddings_amd.weights import (VIT_B16, VIT_L16, VIT_S16, ViTGeometry, f32_to_bf16_bits, infer_vit_geometry, make_vit_weights,
                                               vit_flops_per_crop, vit_geometry_problem, vit_tensor_specs)

SEED = 7
S2 = dataclasses.replace(VIT_S16, num_layers=2)
S3 = dataclasses.replace(VIT_S16, num_layers=3)
L2 = dataclasses.replace(VIT_L16, num_layers=2)
L3 = dataclasses.replace(VIT_L16, num_layers=3, layer_norm_eps=1e-6)
GEOMS = {"S2": S2, "S3": S3, "L2": L2, "L3": L3}


@pytest.fixture(scope="module")
def family_w():
    return {k: make_vit_weights(SEED, g) for k, g in GEOMS.items()}


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
            assert np.array_equal(_bits(got).view(np.uint16), f32_to_bf16_bits(want).reshape(want.shape)), name


def test_presets_and_flop_count():
    assert (VIT_S16.hidden_size, VIT_S16.num_layers, VIT_S16.num_heads, VIT_S16.intermediate_size) == (384, 12, 6, 1536)
    assert (VIT_L16.hidden_size, VIT_L16.num_layers, VIT_L16.num_heads, VIT_L16.intermediate_size) == (1024, 24, 16, 4096)
    for g in (VIT_S16, VIT_B16, VIT_L16):
        assert g.head_dim == 64 and g.seq_len == 197 and g.patch_dim == 768 and vit_geometry_problem(g) is None
    assert vit_flops_per_crop(VIT_B16) == 35126083584
    assert vit_flops_per_crop() == 35126083584
    # the GEMM part is the sum of the launches' 2 M N K
    for g in (VIT_S16, VIT_L16):
        D, F, L = g.hidden_size, g.intermediate_size, g.num_layers
        gemm = 2 * 196 * 768 * D + L * 2 * 197 * (3 * D * D + D * D + 2 * D * F)
        attn = vit_flops_per_crop(g) - gemm
        assert 0 < attn < 0.1 * gemm and attn % L == 0
    assert vit_flops_per_crop(VIT_S16) < vit_flops_per_crop(VIT_B16) < vit_flops_per_crop(VIT_L16)


@pytest.mark.parametrize("key,dtype", [("S2", "float32"), ("S3", "bfloat16"), ("L2", "bfloat16"), ("L3", "float32")])
def test_saved_family_checkpoint_roundtrip(tmp_path, family_w, key, dtype):
    g, w = GEOMS[key], family_w[key]
    ckpt.save_checkpoint(tmp_path, w, "vit", dtype, geometry=g)
    ck = ckpt.read_checkpoint(tmp_path, "vit")
    assert ck.encoder == "vit" and ck.geometry == g
    assert list(ck.tensors) == [n for n, _, _ in vit_tensor_specs(g)]
    _assert_equals_dict(ck, w, dtype)
    assert ck.nbytes == sum(v.size for v in w.values()) * (4 if dtype == "float32" else 2)
    assert infer_vit_geometry(w, eps=g.layer_norm_eps) == g
    # the strict name still refuses what is not ViT-B/16, in its own words
    with pytest.raises(MmeError, match=r"hidden_size = (384|1024), but this library is built for hidden_size = 768"):
        ckpt.read_checkpoint(tmp_path, "vit_b16")


def test_vit_b16_directory_reads_under_both_names(tmp_path):
    g = dataclasses.replace(VIT_B16, num_layers=2)
    w = make_vit_weights(SEED, g)
    ckpt.save_checkpoint(tmp_path, w, "vit", "bfloat16", geometry=g)
    ck = ckpt.read_checkpoint(tmp_path, "vit")
    assert ck.geometry == g
    _assert_equals_dict(ck, w, "bfloat16")
    with pytest.raises(MmeError, match="num_hidden_layers = 2, but this library is built for num_hidden_layers = 12"):
        ckpt.read_checkpoint(tmp_path, "vit_b16")


def test_transformers_vit_large_save_pretrained(tmp_path, family_w):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.ViTConfig(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=2)
    model = transformers.ViTModel(cfg, add_pooling_layer=False)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in family_w["L2"].items()}, strict=True)
    model.save_pretrained(tmp_path)
    ck = ckpt.read_checkpoint(tmp_path, "vit")
    assert ck.geometry == L2
    assert list(ck.tensors) == [n for n, _, _ in vit_tensor_specs(L2)]
    _assert_equals_dict(ck, family_w["L2"], "float32")
    assert any(f.endswith("model.safetensors") for f in ck.source)


def _write_config(tmp_path, **changes):
    cfg = {"model_type": "vit", "image_size": 224, "patch_size": 16, "num_channels": 3, "hidden_size": 1024, "num_hidden_layers": 2,
           "num_attention_heads": 16, "intermediate_size": 4096, "hidden_act": "gelu", "qkv_bias": True, "layer_norm_eps": 1e-12}
    cfg.update(changes)
    (tmp_path / "config.json").write_text(json.dumps(cfg))


@pytest.mark.parametrize("changes,field,value,supported", [
    ({"hidden_size": 512, "num_attention_heads": 8, "intermediate_size": 2048}, "hidden_size", "512", "384, 768, 1024"),
    ({"num_attention_heads": 8}, "num_attention_heads", "8", "16 at hidden_size 1024"),
    ({"patch_size": 14}, "patch_size", "14", "16"),
    ({"image_size": 384}, "image_size", "384", "224"),
    ({"num_hidden_layers": 65}, "num_hidden_layers", "65", "1..64"),
    ({"intermediate_size": 4100}, "intermediate_size", "4100", "a multiple of 64 up to 8192"),
    ({"intermediate_size": 8256}, "intermediate_size", "8256", "a multiple of 64 up to 8192"),
    ({"num_channels": 1}, "num_channels", "1", "3"),
    ({"hidden_size": 1280, "num_attention_heads": 16, "intermediate_size": 5120}, "hidden_size", "1280", "384, 768, 1024"),  # ViT-H: heads of 80
])
def test_unsupported_geometry_names_field_value_and_supported_set(tmp_path, changes, field, value, supported):
    """Refused from config.json alone, before any tensor is read: the directory holds no weights."""
    _write_config(tmp_path, **changes)
    with pytest.raises(MmeError) as e:
        ckpt.read_checkpoint(tmp_path, "vit")
    text = str(e.value)
    assert f"{field} = {value}" in text and "supported" in text and supported in text, text


def test_other_refusals_and_the_command_line(tmp_path, family_w, capsys):
    _write_config(tmp_path, hidden_act="relu")
    with pytest.raises(MmeError, match="hidden_act = 'relu'"):
        ckpt.read_checkpoint(tmp_path, "vit")
    _write_config(tmp_path, hidden_size="1024")
    with pytest.raises(MmeError, match="hidden_size = '1024'; an integer is required"):
        ckpt.read_checkpoint(tmp_path, "vit")
    # a supported configuration whose tensors are another geometry's: the shape check names the tensor
    d = tmp_path / "mixed"
    ckpt.save_checkpoint(d, family_w["S2"], "vit", "float32", geometry=L2)
    with pytest.raises(MmeError, match=r"has shape \(1, 1, 384\), expected \(1, 1, 1024\)"):
        ckpt.read_checkpoint(d, "vit")
    ok = tmp_path / "ok"
    ckpt.save_checkpoint(ok, family_w["S3"], "vit", "bfloat16", geometry=S3)
    assert ckpt.main([str(ok), "--encoder", "vit"]) == 0
    out = capsys.readouterr().out
    assert "encoder     vit" in out and "hidden_size=384" in out and "num_layers=3" in out and "dtype       bfloat16" in out
    assert ckpt.main([str(ok), "--encoder", "vit_b16"]) == 1
    assert "cannot load" in capsys.readouterr().out
    assert "vit" in ckpt.ENCODERS and ViTGeometry() == VIT_B16
