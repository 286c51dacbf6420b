"""SigLIP ViT/16 image towers (196 tokens, tanh-GELU, attention-pooling head) without a GPU: the float64 restatement of
tests/siglip_reference.py against what transformers' own `SiglipVisionModel` returned (tests/golden/siglip_cases.npz,
tests/golden/make_siglip_golden.py); the sigmoid form of tanh-GELU that the GEMM epilogue evaluates; geometry acceptance and
inference; the checkpoint writer and reader (three dtypes, a whole-model directory, both key prefixes); refusals.

Bound of the restatement.  When the fixture was recorded (transformers 5.15.0, float32, eager attention, CPU) the float64
restatement was within max(1 - cos) = 2.51e-13 and max |difference| = 1.42e-6 of the recorded rows over the three recorded
matrices (|value| <= 2.2; per case B16s 2.51e-13 / 1.16e-6, S16 1.76e-13 / 5.34e-7, L16 2.22e-13 / 1.42e-6): the float32
rounding of the model's own arithmetic.  The tests assert 4 x those figures.
"""
import dataclasses
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_siglip_golden as mks  # noqa: E402
import siglip_reference as sr  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import (SIGLIP_B16, SiglipGeometry, infer_siglip_geometry, make_clip_weights, make_siglip_weights,  # noqa: E402
                                               siglip_flops_per_crop, siglip_geometry_problem, siglip_tensor_specs, vit_flops_per_crop)

ONE_MINUS_COS = 4 * 2.51e-13
MAX_ABS = 4 * 1.42e-6
S16 = mks.CASES["S16"][1]
SMALL = dataclasses.replace(S16, num_layers=1, intermediate_size=128)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "siglip_cases.npz"))


@pytest.fixture(scope="module")
def pixels():
    return mks.pixel_values()


@pytest.mark.parametrize("key", list(mks.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, pixels, key):
    seed, geom = mks.CASES[key]
    assert geom.patch_size == 16 and geom.seq_len == 196 and geom.num_layers == 2
    assert sorted(recorded.files) == sorted(f"{k}.pooler_output" for k in mks.CASES)
    w = make_siglip_weights(seed, geom)
    mine = sr.siglip_forward(pixels, w, geom, torch.float64)
    rec = recorded[f"{key}.pooler_output"]
    assert mine.shape == rec.shape == (mks.N_CROPS, geom.hidden_size)
    omc, err = float(sr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{key}: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (key, omc, err)
    # sharpness: the probe added as a residual, the erf-GELU, and two position rows exchanged each leave the bound by orders of magnitude
    hs = sr.siglip_hidden_states(pixels[:4], w, geom, torch.float64)
    probe = torch.from_numpy(w["vision_model.head.probe"].astype(np.float64)).reshape(1, -1)
    wrong = (sr.siglip_head(hs, w, geom, torch.float64) + probe).numpy()
    assert float(sr.one_minus_cos(wrong, rec[:4]).max()) > 1e6 * ONE_MINUS_COS
    sw = dict(w)
    pos = w["vision_model.embeddings.position_embedding.weight"].copy()
    pos[[0, 195]] = pos[[195, 0]]
    sw["vision_model.embeddings.position_embedding.weight"] = pos
    assert float(sr.one_minus_cos(sr.siglip_forward(pixels[:4], sw, geom, torch.float64), rec[:4]).max()) > 100 * ONE_MINUS_COS


def test_tanh_gelu_is_x_times_a_sigmoid():
    """gelu_tanh(x) = x sigmoid(x (c0 + c1 x^2)) with c0 = 2 sqrt(2 / pi), c1 = 0.044715 c0: an identity (0.5 (1 + tanh u) =
    sigmoid(2 u)), so the two agree to the rounding of float64 -- a few ulp of the result, |x| 2^-50 at the most generous."""
    x = torch.cat([torch.linspace(-12, 12, 200_001, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-300, -1e-300], dtype=torch.float64)])
    ref = torch.nn.functional.gelu(x, approximate="tanh")
    mine = sr.gelu_tanh_sigmoid(x)
    assert torch.equal(sr.gelu_tanh(x), 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x**3))))
    err = (mine - ref).abs()
    # where tanh has saturated to -1 in float64 (x < -4.3) the reference is 0 while the sigmoid form keeps its tiny tail,
    # |x| sigmoid < |x| exp(-2 u) < 2^-52 |x| there: absolute room of 2^-50 covers it, relative room of 2^-50 the rest
    tol = 2.0**-50 * torch.maximum(ref.abs(), torch.ones_like(ref))
    print(f"tanh-GELU identity: max |difference| = {float(err.max()):.3g}, max difference / tolerance = {float((err / tol).max()):.3g}")
    assert bool((err <= tol).all())
    inf = torch.tensor([math.inf, -math.inf], dtype=torch.float64)
    got, want = sr.gelu_tanh_sigmoid(inf), torch.nn.functional.gelu(inf, approximate="tanh")
    assert float(got[0]) == math.inf == float(want[0])
    assert float(got[1]) == 0.0 or math.isnan(float(got[1]))  # -inf * 0: the limit is -0, which the device form returns (test_gpu_siglip.py)
    # a fit would not hold this: erf-GELU differs from tanh-GELU by 4.7e-4 in this range
    erf = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    assert float((erf - ref).abs().max()) > 1e-4
    # the constants of csrc/gemm_epilogue.h
    assert sr.C0 == 2.0 * math.sqrt(2.0 / math.pi) and abs(sr.C0 - 1.5957691216057308) < 1e-15 and sr.C1 == 0.044715 * sr.C0


def test_geometry_acceptance_and_inference():
    assert (SIGLIP_B16.hidden_size, SIGLIP_B16.num_layers, SIGLIP_B16.num_heads, SIGLIP_B16.intermediate_size) == (768, 12, 12, 3072)
    assert (SIGLIP_B16.seq_len, SIGLIP_B16.num_patches, SIGLIP_B16.embed_dim, SIGLIP_B16.layer_norm_eps, SIGLIP_B16.hidden_act) == (
        196, 196, 768, 1e-6, "gelu_pytorch_tanh")
    assert siglip_geometry_problem(SIGLIP_B16) is None
    for key in mks.CASES:
        assert siglip_geometry_problem(mks.CASES[key][1]) is None
    r = dataclasses.replace
    assert siglip_geometry_problem(r(SIGLIP_B16, patch_size=14)) == ("patch_size", 14, "16")
    assert siglip_geometry_problem(r(SIGLIP_B16, patch_size=32)) == ("patch_size", 32, "16")
    assert siglip_geometry_problem(r(SIGLIP_B16, image_size=256))[:2] == ("image_size", 256)
    assert siglip_geometry_problem(r(SIGLIP_B16, hidden_size=512, num_heads=8))[:2] == ("hidden_size", 512)
    assert siglip_geometry_problem(r(SIGLIP_B16, hidden_size=1024, num_heads=16))is None
    assert siglip_geometry_problem(r(SIGLIP_B16, hidden_size=1152, num_heads=16))[:2] == ("hidden_size", 1152)
    assert siglip_geometry_problem(r(SIGLIP_B16, hidden_size=1024, num_heads=12))[:2] == ("num_heads", 12)
    assert siglip_geometry_problem(r(SIGLIP_B16, hidden_act="gelu")) == ("hidden_act", "gelu", "gelu_pytorch_tanh")
    assert siglip_geometry_problem(r(SIGLIP_B16, vision_use_head=False))[:2] == ("vision_use_head", False)
    assert siglip_geometry_problem(r(SIGLIP_B16, intermediate_size=4304))[0] == "intermediate_size"
    assert siglip_geometry_problem(r(SIGLIP_B16, num_layers=65))[0] == "num_layers"
    w = make_siglip_weights(3, SMALL)
    shapes = {n: s for n, s, _ in siglip_tensor_specs(SMALL)}
    assert list(w) == list(shapes) and all(w[n].shape == shapes[n] for n in w)
    assert shapes["vision_model.embeddings.position_embedding.weight"] == (196, 384)
    assert shapes["vision_model.head.attention.in_proj_weight"] == (1152, 384) and shapes["vision_model.head.probe"] == (1, 1, 384)
    assert not any("class_embedding" in n or "pre_layrnorm" in n for n in shapes)
    assert infer_siglip_geometry(w) == SMALL
    # the head costs about a sixth of a layer
    layer = (vit_flops_per_crop(SIGLIP_B16) - vit_flops_per_crop(dataclasses.replace(SIGLIP_B16, num_layers=11)))
    head = siglip_flops_per_crop(SIGLIP_B16) - vit_flops_per_crop(SIGLIP_B16)
    assert 0.1 < head / layer < 0.25


MEAN = STD = (0.5, 0.5, 0.5)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_save_then_read_round_trip(tmp_path, dtype):
    w = make_siglip_weights(5, SMALL)
    ckpt.save_checkpoint(tmp_path, w, "siglip", dtype, geometry=SMALL, image_mean=MEAN, image_std=STD, image_processor_type="SiglipImageProcessor")
    cfg = json.load(open(os.path.join(tmp_path, "config.json")))
    assert cfg["hidden_act"] == "gelu_pytorch_tanh" and cfg["patch_size"] == 16 and cfg["model_type"] == "siglip_vision_model"
    ck = ckpt.read_checkpoint(tmp_path, "siglip")
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    assert ck.encoder == "siglip" and ck.geometry == SMALL and ck.geometry.seq_len == 196 and ck.dtype == dtype
    assert ck.image_mean == MEAN and ck.image_std == STD
    assert list(ck.tensors) == [n for n, _, _ in siglip_tensor_specs(SMALL)]
    for name, t in ck.tensors.items():
        want = torch.from_numpy(w[name]).to(tdt)
        assert t.dtype == tdt and t.shape == want.shape and torch.equal(t.float(), want.float()), name
    assert ckpt.main([str(tmp_path), "--encoder", "siglip_vit"]) == 0


def _save_state(path, tensors):
    from safetensors.torch import save_file

    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})


def _rewrite_config(path, fn):
    p = os.path.join(path, "config.json")
    cfg = json.load(open(p))
    fn(cfg)
    json.dump(cfg, open(p, "w"))


def test_whole_model_directory_and_both_key_prefixes(tmp_path, caplog):
    w = make_siglip_weights(5, SMALL)
    ckpt.save_checkpoint(tmp_path, w, "siglip", "float32", geometry=SMALL)
    plain = ckpt.read_checkpoint(tmp_path, "siglip")
    # the tower's own keys, as SiglipVisionModel.save_pretrained of transformers 5 writes them
    _save_state(tmp_path, {k[len("vision_model."):]: v for k, v in w.items()})
    bare = ckpt.read_checkpoint(tmp_path, "siglip")
    assert list(bare.tensors) == list(plain.tensors) and all(torch.equal(bare.tensors[k], plain.tensors[k]) for k in plain.tensors)
    # a whole SiglipModel: vision_config / text_config, text tensors, logit_scale and logit_bias beside the tower
    whole = dict(w)
    whole.update({"text_model.embeddings.token_embedding.weight": np.zeros((8, 16), np.float32), "text_model.head.weight": np.zeros((4, 4), np.float32),
                  "text_model.embeddings.position_ids": np.zeros((1, 64), np.float32), "logit_scale": np.ones((1,), np.float32),
                  "logit_bias": np.ones((1,), np.float32)})
    _save_state(tmp_path, whole)
    _rewrite_config(tmp_path, lambda c: (vc := dict(c), c.clear(), c.update(model_type="siglip", vision_config=vc, text_config={"hidden_size": 16})))
    ck = ckpt.read_checkpoint(tmp_path, "siglip")
    assert ck.geometry == SMALL and list(ck.tensors) == list(plain.tensors)
    assert all(torch.equal(ck.tensors[k], plain.tensors[k]) for k in plain.tensors)
    # a preprocessor file that asks for SigLIP's own plain resize: mean / std are taken, the offline check says what K1 does instead
    json.dump({"image_processor_type": "SiglipImageProcessor", "do_rescale": True, "rescale_factor": 1 / 255, "do_normalize": True, "resample": 3,
               "size": {"height": 224, "width": 224}, "image_mean": list(MEAN), "image_std": list(STD)},
              open(os.path.join(tmp_path, "preprocessor_config.json"), "w"))
    import logging

    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(tmp_path, "siglip")
    assert ck.image_mean == MEAN and ck.image_std == STD
    assert any("does not keep the aspect" in r.getMessage() and "SiglipImageProcessor" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("change, message", [
    (dict(patch_size=14), r"patch_size = 14; supported: 16"),
    (dict(image_size=256), r"image_size = 256; supported: 224"),
    (dict(hidden_size=512, num_attention_heads=8), r"hidden_size = 512; supported: 384, 768, 1024"),
    (dict(hidden_size=1280, num_attention_heads=16), r"hidden_size = 1280; supported: 384, 768, 1024"),
    (dict(hidden_size=384, num_attention_heads=4), r"num_attention_heads = 4; supported: 6 at hidden_size 384 \(heads of 64\)"),
    (dict(hidden_act="gelu"), r"hidden_act = 'gelu'; supported: gelu_pytorch_tanh"),
    (dict(vision_use_head=False), r"vision_use_head = False; supported: True"),
])
def test_refusals_name_the_field(tmp_path, change, message):
    ckpt.save_checkpoint(tmp_path, make_siglip_weights(7, SMALL), "siglip", "float32", geometry=SMALL)
    _rewrite_config(tmp_path, lambda c: c.update(change))
    with pytest.raises(MmeError, match=message):
        ckpt.read_checkpoint(tmp_path, "siglip")
    assert ckpt.main([str(tmp_path), "--encoder", "siglip_vit"]) == 1


def test_heads_of_80_are_refused(tmp_path):
    # 1280 / 16 = 80 is refused at the width already; heads of 80 at a supported width cannot divide it: 1024 / 80 is no integer,
    # so the nearest statement is a head count whose heads are not 64 wide
    ckpt.save_checkpoint(tmp_path, make_siglip_weights(7, SMALL), "siglip", "float32", geometry=SMALL)
    _rewrite_config(tmp_path, lambda c: c.update(hidden_size=1024, num_attention_heads=13))
    with pytest.raises(MmeError, match=r"num_attention_heads = 13; supported: 16 at hidden_size 1024 \(heads of 64\)"):
        ckpt.read_checkpoint(tmp_path, "siglip")


def test_missing_and_misshaped_tensors_are_named(tmp_path):
    w = make_siglip_weights(7, SMALL)
    ckpt.save_checkpoint(tmp_path, w, "siglip", "float32", geometry=SMALL)
    less = {k: v for k, v in w.items() if k != "vision_model.head.probe"}
    _save_state(tmp_path, less)
    with pytest.raises(MmeError, match=r"tensor 'vision_model.head.probe' is missing"):
        ckpt.read_checkpoint(tmp_path, "siglip")
    bad = dict(w)
    bad["vision_model.head.attention.in_proj_weight"] = np.zeros((768, 384), np.float32)
    _save_state(tmp_path, bad)
    with pytest.raises(MmeError, match=r"in_proj_weight' has shape \(768, 384\), expected \(1152, 384\)"):
        ckpt.read_checkpoint(tmp_path, "siglip")
    bad = dict(w)
    bad["vision_model.embeddings.position_embedding.weight"] = np.zeros((197, 384), np.float32)
    _save_state(tmp_path, bad)
    with pytest.raises(MmeError, match=r"position_embedding.weight' has shape \(197, 384\), expected \(196, 384\)"):
        ckpt.read_checkpoint(tmp_path, "siglip")


def test_the_clip_encoder_still_refuses_a_siglip_directory_and_siglip_a_clip_one(tmp_path):
    ckpt.save_checkpoint(tmp_path, make_siglip_weights(7, SMALL), "siglip", "float32", geometry=SMALL)
    with pytest.raises(MmeError, match=r"config.json: hidden_act = 'gelu_pytorch_tanh'; supported: gelu, quick_gelu"):
        ckpt.read_checkpoint(tmp_path, "clip")
    from multimodal_embeddings_amd.weights import CLIPGeometry

    cg = CLIPGeometry(hidden_size=384, num_layers=1, num_heads=6, intermediate_size=128, projection_dim=None)
    cdir = os.path.join(tmp_path, "clip")
    ckpt.save_checkpoint(cdir, make_clip_weights(7, cg), "clip", "float32", geometry=cg)
    with pytest.raises(MmeError, match=r"hidden_act = 'quick_gelu'; supported: gelu_pytorch_tanh"):
        ckpt.read_checkpoint(cdir, "siglip")
    assert "siglip" in ckpt.ENCODERS and "siglip" in ckpt.CLIP_RULE_ENCODERS


def test_embedder_refuses_another_pool_before_it_touches_a_device():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(ValueError, match=r"pool = 'last': encoder='siglip_vit' pools with the tower's attention-pooling head"):
        RegionEmbedder(encoder="siglip_vit", pool="last")


def test_the_two_surfaces_that_spell_it_siglip_vit():
    """RegionEmbedder and the command line have always refused the bare name "siglip" and still do; they take "siglip_vit"."""
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    assert "siglip" in ckpt.ENCODERS and "siglip_vit" in ckpt.CLI_ENCODERS and "siglip" not in ckpt.CLI_ENCODERS
    with pytest.raises(ValueError, match="'siglip_vit'"):
        RegionEmbedder(encoder="siglip")
    with pytest.raises(SystemExit):
        ckpt.main(["--encoder", "siglip", "x"])
    assert ckpt.main(["--encoder", "siglip_vit", "no-such-directory"]) == 1
