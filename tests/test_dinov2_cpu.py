"""DINOv2 ViT/14 image towers (257 tokens, LayerScale, `pooler_output`) without a GPU: the float64 restatement of
tests/dinov2_reference.py against what transformers' own `Dinov2Model` returned (tests/golden/dinov2_cases.npz,
tests/golden/make_dinov2_golden.py); the loader's position interpolation against the model's own, bit for bit; the retile
mapping of csrc/dinov2.hip in numpy against the patch-14 im2col; geometry acceptance and inference; the checkpoint writer and
reader (three dtypes, the 1370-row table, the prefixed keys); refusals; the ABI.

Bound of the restatement.  When the fixture was recorded (transformers 5.15.0, float32, eager attention, CPU) the float64
restatement was within max(1 - cos) = 3.42e-13 and max |difference| = 5.43e-6 of the recorded rows over the four recorded
matrices (|value| <= 5.6; per case S14 2.86e-13 / 5.43e-6, B14 3.34e-13 / 5.02e-6, L14 3.42e-13 / 4.92e-6, S14p37 3.07e-13 /
4.19e-6): the float32 rounding of the model's own arithmetic.  The tests assert 4 x those figures.
"""
import dataclasses
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import dinov2_reference as dr  # noqa: E402
import make_dinov2_golden as mkd  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import (DINOV2_B14, DINOV2_L14, DINOV2_S14, SUPPORTED_VIT, Dinov2Geometry, dinov2_flops_per_crop,  # noqa: E402
                                               dinov2_geometry_problem, dinov2_tensor_specs, infer_dinov2_geometry, make_dinov2_weights,
                                               vit_geometry_problem)

ONE_MINUS_COS = 4 * 3.42e-13
MAX_ABS = 4 * 5.43e-6
S14 = mkd.CASES["S14"][1]
SMALL = dataclasses.replace(S14, num_layers=1, intermediate_size=128)
POS = "embeddings.position_embeddings"


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "dinov2_cases.npz"))


@pytest.fixture(scope="module")
def pixels():
    return mkd.pixel_values()


@pytest.mark.parametrize("key", list(mkd.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, pixels, key):
    seed, geom, grid = mkd.CASES[key]
    assert geom.patch_size == 14 and geom.seq_len == 257 and geom.num_patches == 256 and geom.num_layers == 2
    assert sorted(recorded.files) == sorted(f"{k}.pooler_output" for k in mkd.CASES)
    w = make_dinov2_weights(seed, geom, pos_grid=grid)
    assert w[POS].shape == (1, 1 + grid * grid, geom.hidden_size)
    mine = dr.dinov2_forward(pixels, w, geom, torch.float64)
    rec = recorded[f"{key}.pooler_output"]
    assert mine.shape == rec.shape == (mkd.N_CROPS, geom.hidden_size)
    omc, err = float(dr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{key}: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (key, omc, err)
    # sharpness: two position rows exchanged, and layer_scale2 dropped, each leave the bound by 100 x and more
    for mutant in ("swap_pos", "no_layer_scale2"):
        wrong = dr.dinov2_forward(pixels[:4], w, geom, torch.float64, mutate=mutant)
        far = float(dr.one_minus_cos(wrong, rec[:4]).max())
        print(f"{key}: {mutant}: max(1 - cos) = {far:.3g}")
        assert far >= 100 * ONE_MINUS_COS, (key, mutant, far)


@pytest.mark.parametrize("grid, D", [(37, 384), (37, 1024), (16, 384), (24, 768)])
def test_loader_interpolation_equals_the_models_own_bit_for_bit(grid, D):
    from transformers import Dinov2Config
    from transformers.models.dinov2.modeling_dinov2 import Dinov2Embeddings

    g = torch.Generator().manual_seed(grid * 1000 + D)
    table = torch.randn(1, 1 + grid * grid, D, generator=g)
    emb = Dinov2Embeddings(Dinov2Config(hidden_size=D, num_attention_heads=D // 64, image_size=14 * grid, patch_size=14))
    with torch.no_grad():
        emb.position_embeddings.copy_(table)
        want = emb.interpolate_pos_encoding(torch.zeros(1, 257, D), 224, 224)[0]
    got = ckpt.interpolate_dinov2_positions(table)
    assert got.dtype == torch.float32 and tuple(got.shape) == (257, D) and got.is_contiguous()
    assert torch.equal(got, want)
    assert torch.equal(got[0], table[0, 0])  # the class row is kept as it is
    assert torch.equal(got, dr.position_table({POS: table.numpy()}))
    if grid == 16:
        assert torch.equal(got, table[0])  # a 257-row table is taken as it is
    # a bf16 or f16 table is widened, interpolated in float32 and stays float32 (the device holds the table as f32)
    half = ckpt.interpolate_dinov2_positions(table.to(torch.bfloat16))
    assert half.dtype == torch.float32 and torch.equal(half, ckpt.interpolate_dinov2_positions(table.to(torch.bfloat16).float()))


def test_position_table_that_is_no_square_grid_is_refused_naming_the_tensor(tmp_path):
    with pytest.raises(MmeError, match=r"tensor 'embeddings.position_embeddings' has 300 rows: the patch part \(299 rows\) is no square grid"):
        ckpt.interpolate_dinov2_positions(torch.zeros(1, 300, 384))
    w = make_dinov2_weights(7, SMALL)
    w[POS] = np.zeros((1, 300, 384), np.float32)
    with pytest.raises(ValueError, match=r"tensor 'embeddings.position_embeddings' has 300 rows"):
        infer_dinov2_geometry(w)
    ckpt.save_checkpoint(tmp_path, make_dinov2_weights(7, SMALL), "dinov2", "float32", geometry=SMALL)
    _save_state(tmp_path, w)
    with pytest.raises(MmeError, match=r"tensor 'embeddings.position_embeddings' has shape \(1, 300, 384\): the patch part \(299 rows\) is no square grid"):
        ckpt.read_checkpoint(tmp_path, "dinov2")


def _patchify(x, p):
    n, c, h, w = x.shape
    g = h // p
    return x.reshape(n, c, g, p, g, p).transpose(0, 2, 4, 1, 3, 5).reshape(n * g * g, c * p * p)


def test_retile_mapping_is_the_patch14_im2col_of_the_same_pixels():
    rng = np.random.default_rng(3)
    px = rng.standard_normal((3, 3, 224, 224)).astype(np.float32)
    px[0] = np.arange(3 * 224 * 224, dtype=np.float32).reshape(3, 224, 224)  # every value once: a permutation is visible
    p16 = _patchify(px, 16)
    assert p16.shape == (3 * 196, 768)
    got = dr.retile_p14_reference(p16)
    assert got.shape == (3 * 256, 640) and got.dtype == p16.dtype
    want = np.zeros((3 * 256, 640), np.float32)
    want[:, :588] = _patchify(px, 14)
    assert np.array_equal(got, want)
    assert not got[:, 588:].any()
    # a permutation of the 150 528 values of a crop
    assert np.array_equal(np.sort(got[:256, :588].ravel()), np.sort(p16[:196].ravel())) and got[:256, :588].size == 150528
    # a transposed patch grid (PX major) or a transposed patch (kx major) is caught
    t_grid = want.reshape(3, 16, 16, 640).transpose(0, 2, 1, 3).reshape(3 * 256, 640)
    t_patch = want.copy()
    t_patch[:, :588] = want[:, :588].reshape(-1, 3, 14, 14).transpose(0, 1, 3, 2).reshape(-1, 588)
    assert not np.array_equal(got, t_grid) and not np.array_equal(got, t_patch)
    # bf16 bit patterns travel unchanged
    bits = rng.integers(0, 65536, size=(196, 768), dtype=np.uint16)
    out = dr.retile_p14_reference(bits)
    assert out.dtype == np.uint16 and np.array_equal(np.sort(out[:, :588].ravel()), np.sort(bits.ravel()))


def test_geometry_acceptance_and_inference():
    assert (DINOV2_S14.hidden_size, DINOV2_S14.num_layers, DINOV2_S14.num_heads, DINOV2_S14.intermediate_size) == (384, 12, 6, 1536)
    assert (DINOV2_B14.hidden_size, DINOV2_B14.num_layers, DINOV2_B14.num_heads, DINOV2_B14.intermediate_size) == (768, 12, 12, 3072)
    assert (DINOV2_L14.hidden_size, DINOV2_L14.num_layers, DINOV2_L14.num_heads, DINOV2_L14.intermediate_size) == (1024, 24, 16, 4096)
    for g in (DINOV2_S14, DINOV2_B14, DINOV2_L14):
        assert (g.image_size, g.patch_size, g.grid, g.num_patches, g.seq_len, g.patch_dim, g.patch_dim_padded) == (224, 14, 16, 256, 257, 588, 640)
        assert (g.layer_norm_eps, g.hidden_act, g.embed_dim, g.position_rows) == (1e-6, "gelu", g.hidden_size, 257)
        assert dinov2_geometry_problem(g) is None
        # the ViT, CLIP and SigLIP loaders keep refusing the geometry
        assert vit_geometry_problem(g) == ("patch_size", 14, "16, 32")
    assert SUPPORTED_VIT["patch_size"] == (16, 32)
    r = dataclasses.replace
    assert dinov2_geometry_problem(r(DINOV2_B14, use_swiglu_ffn=True))[:2] == ("use_swiglu_ffn", True)
    assert dinov2_geometry_problem(r(DINOV2_B14, num_register_tokens=4))[:2] == ("num_register_tokens", 4)
    assert dinov2_geometry_problem(r(DINOV2_B14, patch_size=16)) == ("patch_size", 16, "14")
    assert dinov2_geometry_problem(r(DINOV2_B14, image_size=518))[:2] == ("image_size", 518)
    assert dinov2_geometry_problem(r(DINOV2_B14, hidden_size=1536, num_heads=24))[:2] == ("hidden_size", 1536)
    assert dinov2_geometry_problem(r(DINOV2_B14, num_heads=8))[:2] == ("num_heads", 8)
    assert dinov2_geometry_problem(r(DINOV2_B14, intermediate_size=3000))[0] == "intermediate_size"
    assert dinov2_geometry_problem(r(DINOV2_L14, intermediate_size=8256))[0] == "intermediate_size"
    assert dinov2_geometry_problem(r(DINOV2_B14, num_layers=65))[0] == "num_layers"
    assert dinov2_geometry_problem(r(DINOV2_B14, num_layers=0))[0] == "num_layers"
    assert dinov2_geometry_problem(r(DINOV2_B14, hidden_act="quick_gelu")) == ("hidden_act", "quick_gelu", "gelu")
    for grid in (16, 37):
        w = make_dinov2_weights(3, SMALL, pos_grid=grid)
        geom = r(SMALL, position_grid=grid)
        shapes = {n: s for n, s, _ in dinov2_tensor_specs(geom)}
        assert list(w) == list(shapes) and all(w[n].shape == shapes[n] for n in w)
        assert shapes[POS] == (1, 1 + grid * grid, 384) and shapes["embeddings.patch_embeddings.projection.weight"] == (384, 3, 14, 14)
        assert "embeddings.mask_token" not in shapes and shapes["encoder.layer.0.layer_scale2.lambda1"] == (384,)
        assert infer_dinov2_geometry(w) == geom
    # the seeded LayerScale is spread over about [0.05, 2], bf16-representable, far from a constant
    lam = make_dinov2_weights(3, S14)["encoder.layer.1.layer_scale1.lambda1"]
    assert 0.05 <= lam.min() < 0.5 and 1.6 < lam.max() <= 2.0 and lam.std() > 0.2
    assert np.array_equal(lam.view(np.uint32) & 0xFFFF, np.zeros(lam.shape, np.uint32))
    # 257 tokens cost about 1.3 x the 197 of the same width
    from multimodal_embeddings_amd.weights import VIT_B16, vit_flops_per_crop

    assert 1.28 < dinov2_flops_per_crop(DINOV2_B14) / vit_flops_per_crop(VIT_B16) < 1.36


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _save_state(path, tensors):
    from safetensors.torch import save_file

    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})


def _rewrite_config(path, fn):
    p = os.path.join(path, "config.json")
    cfg = json.load(open(p))
    fn(cfg)
    json.dump(cfg, open(p, "w"))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("grid", [16, 37])
def test_save_then_read_round_trip(tmp_path, dtype, grid):
    w = make_dinov2_weights(5, SMALL, pos_grid=grid)
    geom = dataclasses.replace(SMALL, position_grid=grid)
    ckpt.save_checkpoint(tmp_path, w, "dinov2", dtype, geometry=geom, image_mean=MEAN, image_std=STD, image_processor_type="BitImageProcessor")
    cfg = json.load(open(os.path.join(tmp_path, "config.json")))
    assert cfg["model_type"] == "dinov2" and cfg["patch_size"] == 14 and cfg["image_size"] == 14 * grid and cfg["hidden_act"] == "gelu"
    assert cfg["mlp_ratio"] * cfg["hidden_size"] == 128 and cfg["use_swiglu_ffn"] is False and cfg["layer_norm_eps"] == 1e-6
    ck = ckpt.read_checkpoint(tmp_path, "dinov2")
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    assert ck.encoder == "dinov2" and ck.geometry == geom and ck.geometry.seq_len == 257 and ck.dtype == dtype
    assert ck.image_mean == MEAN and ck.image_std == STD
    assert list(ck.tensors) == [n for n, _, _ in dinov2_tensor_specs(geom)]
    for name, t in ck.tensors.items():
        want = torch.from_numpy(w[name]).to(tdt)
        assert t.dtype == tdt and t.shape == want.shape and torch.equal(t.float(), want.float()), name
    # the table the device will hold: interpolated once, float32 under every dtype
    table = ck.extra["position_table"]
    assert table.dtype == torch.float32 and tuple(table.shape) == (257, 384)
    assert torch.equal(table, ckpt.interpolate_dinov2_positions(torch.from_numpy(w[POS])))  # the seeded values are bf16-representable
    assert ckpt.main([str(tmp_path), "--encoder", "dinov2"]) == 0


def test_prefixed_keys_mask_token_and_the_offline_check(tmp_path, caplog):
    w = make_dinov2_weights(5, SMALL, pos_grid=37)
    geom = dataclasses.replace(SMALL, position_grid=37)
    ckpt.save_checkpoint(tmp_path, w, "dinov2", "float32", geometry=geom)
    plain = ckpt.read_checkpoint(tmp_path, "dinov2")
    # Dinov2ForImageClassification: the model under "dinov2.", a classifier beside it; mask_token is read past
    pre = {"dinov2." + k: v for k, v in w.items()}
    pre.update({"dinov2.embeddings.mask_token": np.ones((1, 384), np.float32), "classifier.weight": np.zeros((10, 768), np.float32),
                "classifier.bias": np.zeros((10,), np.float32)})
    _save_state(tmp_path, pre)
    ck = ckpt.read_checkpoint(tmp_path, "dinov2")
    assert list(ck.tensors) == list(plain.tensors) and all(torch.equal(ck.tensors[k], plain.tensors[k]) for k in plain.tensors)
    assert ckpt.canonical_dinov2_name("embeddings.mask_token") is None and ckpt.canonical_dinov2_name("dinov2.layernorm.bias") == "layernorm.bias"
    # DINOv2's own preprocessing (shortest edge 256 + centre crop) is out of scope: mean / std are taken, the offline check says so
    json.dump({"image_processor_type": "BitImageProcessor", "do_rescale": True, "rescale_factor": 1 / 255, "do_normalize": True, "resample": 3,
               "size": {"shortest_edge": 256}, "do_center_crop": True, "crop_size": {"height": 224, "width": 224}, "image_mean": list(MEAN),
               "image_std": list(STD)}, open(os.path.join(tmp_path, "preprocessor_config.json"), "w"))
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(tmp_path, "dinov2")
    assert ck.image_mean == MEAN and ck.image_std == STD
    assert any("shortest-edge-256" in r.getMessage() and "K1 does not run that rule" in r.getMessage() for r in caplog.records)
    assert ckpt.main([str(tmp_path), "--encoder", "dinov2"]) == 0
    assert "dinov2" in ckpt.ENCODERS and "dinov2" in ckpt.CLI_ENCODERS and "dinov2" in ckpt.CLIP_RULE_ENCODERS


@pytest.mark.parametrize("change, message", [
    (dict(use_swiglu_ffn=True), r"use_swiglu_ffn = True; supported: False"),
    (dict(patch_size=16), r"patch_size = 16; supported: 14"),
    (dict(hidden_size=1536, num_attention_heads=24), r"hidden_size = 1536; supported: 384, 768, 1024"),
    (dict(hidden_size=384, num_attention_heads=4), r"num_attention_heads = 4; supported: 6 at hidden_size 384 \(heads of 64\)"),
    (dict(hidden_size=1024, num_attention_heads=16, mlp_ratio=9), r"mlp_ratio = 9 at hidden_size = 1024 \(an MLP of 9216\); supported: mlp_ratio x hidden_size a multiple of 64 up to 8192"),
    (dict(mlp_ratio=0.9), r"mlp_ratio = 0.9 at hidden_size = 384 \(an MLP of 345\); supported: mlp_ratio x hidden_size a multiple of 64 up to 8192"),
    (dict(num_hidden_layers=65), r"num_hidden_layers = 65; supported: 1..64"),
    (dict(num_hidden_layers=0), r"num_hidden_layers = 0; supported: 1..64"),
    (dict(hidden_act="quick_gelu"), r"hidden_act = 'quick_gelu'; supported: gelu"),
    (dict(model_type="dinov2_with_registers", num_register_tokens=4), r"model_type = 'dinov2_with_registers', num_register_tokens = 4; supported: dinov2 with num_register_tokens = 0"),
    (dict(num_register_tokens=4), r"num_register_tokens = 4; supported: dinov2 with num_register_tokens = 0"),
])
def test_refusals_name_the_field(tmp_path, change, message):
    ckpt.save_checkpoint(tmp_path, make_dinov2_weights(7, SMALL), "dinov2", "float32", geometry=SMALL)
    _rewrite_config(tmp_path, lambda c: c.update(change))
    with pytest.raises(MmeError, match=message):
        ckpt.read_checkpoint(tmp_path, "dinov2")
    assert ckpt.main([str(tmp_path), "--encoder", "dinov2"]) == 1


def test_missing_and_misshaped_tensors_are_named(tmp_path):
    w = make_dinov2_weights(7, SMALL)
    ckpt.save_checkpoint(tmp_path, w, "dinov2", "float32", geometry=SMALL)
    _save_state(tmp_path, {k: v for k, v in w.items() if k != "encoder.layer.0.layer_scale2.lambda1"})
    with pytest.raises(MmeError, match=r"tensor 'encoder.layer.0.layer_scale2.lambda1' is missing"):
        ckpt.read_checkpoint(tmp_path, "dinov2")
    bad = dict(w)
    bad["embeddings.patch_embeddings.projection.weight"] = np.zeros((384, 3, 16, 16), np.float32)
    _save_state(tmp_path, bad)
    with pytest.raises(MmeError, match=r"projection.weight' has shape \(384, 3, 16, 16\), expected \(384, 3, 14, 14\)"):
        ckpt.read_checkpoint(tmp_path, "dinov2")


def test_the_other_loaders_keep_refusing_patch_14(tmp_path):
    ckpt.save_checkpoint(tmp_path, make_dinov2_weights(7, SMALL), "dinov2", "float32", geometry=SMALL)
    _rewrite_config(tmp_path, lambda c: c.update(image_size=224, intermediate_size=128))
    with pytest.raises(MmeError, match=r"patch_size = 14; supported: 16, 32"):
        ckpt.read_checkpoint(tmp_path, "vit")
    with pytest.raises(MmeError, match=r"patch_size = 14; supported: 16, 32"):
        ckpt.read_checkpoint(tmp_path, "clip")
    with pytest.raises(MmeError, match=r"patch_size = 14; supported: 16"):
        ckpt.read_checkpoint(tmp_path, "siglip")


def test_embedder_knows_the_encoder_and_has_no_text_tower():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(ValueError, match="'dinov2' \\(a DINOv2 ViT/14 image tower\\)"):
        RegionEmbedder(encoder="dino")
    e = RegionEmbedder.__new__(RegionEmbedder)
    e.encoder, e._text_source, e.engines, e.checkpoint = "dinov2", None, [None], None
    with pytest.raises(NotImplementedError, match="a DINOv2 tower is trained on images alone and has no text tower"):
        e._load_text_tower()
    e._text_source = True
    with pytest.raises(NotImplementedError):
        e._load_text_tower()


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "mme.h")).read()
    for name in ("mme_load_dinov2", "mme_load_dinov2_as", "mme_dinov2_apply"):
        assert name in EXPORTS and f"int {name}(" in header
    assert "#define MME_ABI_VERSION 2" in header and "} mme_dinov2_weights;" in header and "} mme_dinov2_scale;" in header
    assert "kind (0 ViT, 1 CLIP, 2 SigLIP, 3 DINOv2)" in header
    for m in ("load_dinov2", "load_dinov2_checkpoint", "dinov2_apply"):
        assert callable(getattr(Engine, m))
    assert Engine.DINOV2_OPS == {"retile": 0, "embed_rows": 1, "attention": 2, "pool_ln_l2": 3, "rowscale": 4, "mul": 5}
    # the ctypes structs have the header's layout: 16 pointers, two int64, six int32 and a float
    from multimodal_embeddings_amd import _lib

    import ctypes as C

    assert C.sizeof(_lib._Dinov2ApplyArgs) == 16 * 8 + 2 * 8 + 6 * 4 + 4 + 4 and C.sizeof(_lib._Dinov2Scale) == 16
    assert C.sizeof(_lib._Dinov2Weights) == C.sizeof(_lib._Weights) + 8
