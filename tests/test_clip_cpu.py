"""The CLIP image-tower encoder without a GPU: the float64 restatement (tests/clip_reference.py) against what transformers'
own classes returned (tests/golden/clip_cases.npz, tests/golden/make_clip_golden.py) and, where transformers imports,
against the live classes; the checkpoint directory reader and writer for encoder "clip".

Bound of the restatement.  When the fixture was recorded (transformers 5.15.0, float32, eager attention) the float64
restatement was within max(1 - cos) = 2.27e-13 and max |difference| = 2.64e-6 of the recorded rows over the seven recorded
matrices (|value| <= 5.65): the float32 rounding of the model's own arithmetic.  The tests assert 4 x those figures.
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

import clip_reference as cr  # noqa: E402
import make_clip_golden as mk  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, CLIPGeometry, clip_flops_per_crop, clip_tensor_specs, make_clip_weights, make_vit_weights,  # noqa: E402
                                               round_to_bf16, vit_flops_per_crop)

ONE_MINUS_COS = 4 * 2.27e-13
MAX_ABS = 4 * 2.64e-6
S2 = mk.CASES["S2"][1]


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "clip_cases.npz"))


@pytest.fixture(scope="module")
def pixels():
    return mk.pixel_values()


def _close(mine, rec, what):
    omc, err = float(cr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{what}: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (what, omc, err)


@pytest.mark.parametrize("key", list(mk.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, pixels, key):
    seed, geom = mk.CASES[key]
    w = make_clip_weights(seed, geom)
    pooled, proj = cr.clip_forward(pixels, w, geom, torch.float64)
    _close(pooled, recorded[f"{key}.pooler_output"], f"{key}.pooler_output")
    assert (proj is not None) == bool(geom.projection_dim) == (f"{key}.image_embeds" in recorded.files)
    if proj is not None:
        assert proj.shape == (mk.N_CROPS, geom.projection_dim)
        _close(proj, recorded[f"{key}.image_embeds"], f"{key}.image_embeds")
    # sharpness: the same tower with the other activation, and with pre_layrnorm's weight and bias exchanged, is far outside
    other = dataclasses.replace(geom, hidden_act="gelu" if geom.hidden_act == "quick_gelu" else "quick_gelu")
    assert float(cr.one_minus_cos(cr.clip_forward(pixels[:4], w, other, torch.float64)[0], recorded[f"{key}.pooler_output"][:4]).max()) > 1e-6
    sw = dict(w)
    sw["vision_model.pre_layrnorm.weight"], sw["vision_model.pre_layrnorm.bias"] = w["vision_model.pre_layrnorm.bias"], w["vision_model.pre_layrnorm.weight"]
    assert float(cr.one_minus_cos(cr.clip_forward(pixels[:4], sw, geom, torch.float64)[0], recorded[f"{key}.pooler_output"][:4]).max()) > 1e-3


@pytest.mark.parametrize("key", ["S2", "B2"])
def test_restatement_agrees_with_the_live_class(pixels, key):
    pytest.importorskip("transformers")
    seed, geom = mk.CASES[key]
    w = make_clip_weights(seed, geom)
    model = mk.hf_model(geom, w)
    with torch.no_grad():
        res = model(pixel_values=torch.from_numpy(pixels))
    pooled, proj = cr.clip_forward(pixels, w, geom, torch.float64)
    if geom.projection_dim:
        _close(proj, res.image_embeds.numpy(), f"live {key}.image_embeds")
    else:
        _close(pooled, res.pooler_output.numpy(), f"live {key}.pooler_output")


def test_seeded_weights_and_flops():
    w = make_clip_weights(3, S2)
    assert [n for n, _, _ in clip_tensor_specs(S2)] == list(w) and len(w) == 5 + 16 * 2 + 2 + 1
    for name, shape, kind in clip_tensor_specs(S2):
        assert w[name].shape == tuple(shape) and np.array_equal(round_to_bf16(w[name]), w[name]), name
        if kind == "gamma":  # away from 1: a dropped LayerNorm weight shows
            assert 0.15 < float(np.abs(w[name] - 1).mean()) < 0.3, name
        if kind == "bias" and "norm" in name:
            assert 0.05 < float(np.abs(w[name]).mean()) < 0.12, name
    assert "vision_model.embeddings.patch_embedding.bias" not in w
    assert np.array_equal(make_clip_weights(3, S2)["visual_projection.weight"], w["visual_projection.weight"])
    assert not np.array_equal(make_clip_weights(4, S2)["visual_projection.weight"], w["visual_projection.weight"])
    assert (CLIP_B16.hidden_size, CLIP_B16.num_layers, CLIP_B16.num_heads, CLIP_B16.intermediate_size) == (768, 12, 12, 3072)
    assert (CLIP_B16.projection_dim, CLIP_B16.hidden_act, CLIP_B16.layer_norm_eps, CLIP_B16.embed_dim) == (512, "quick_gelu", 1e-5, 512)
    assert clip_flops_per_crop(CLIP_B16) == vit_flops_per_crop(CLIP_B16) + 2 * 768 * 512
    assert clip_flops_per_crop(dataclasses.replace(CLIP_B16, projection_dim=None)) == vit_flops_per_crop(CLIP_B16)


def test_clip_is_an_encoder():
    assert "clip" in ckpt.ENCODERS
    with pytest.raises(SystemExit):
        ckpt.main(["--encoder", "siglip", "x"])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_save_then_read_returns_every_tensor_bit_for_bit(tmp_path, dtype):
    w = make_clip_weights(5, S2)
    ckpt.save_checkpoint(tmp_path, w, "clip", dtype, geometry=S2, image_mean=(0.5, 0.4, 0.3), image_std=(0.2, 0.25, 0.3))
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    assert ck.encoder == "clip" and ck.geometry == S2 and ck.dtype == dtype and ck.image_mean == (0.5, 0.4, 0.3)
    assert list(ck.tensors) == [n for n, _, _ in clip_tensor_specs(S2)]
    for name, t in ck.tensors.items():
        want = torch.from_numpy(w[name]).to(tdt)
        assert t.dtype == tdt and t.shape == want.shape and torch.equal(t.view(torch.int16 if tdt != torch.float32 else torch.int32),
                                                                         want.view(torch.int16 if tdt != torch.float32 else torch.int32)), name
    assert ckpt.main([str(tmp_path), "--encoder", "clip"]) == 0


def test_saved_directory_loads_into_transformers(tmp_path, pixels):
    tf = pytest.importorskip("transformers")
    w = make_clip_weights(12, S2)
    ckpt.save_checkpoint(tmp_path, w, "clip", "float32", geometry=S2)
    model, info = tf.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    assert model.config.hidden_act == "gelu" and model.config.projection_dim == 256
    with torch.no_grad():
        e = model.float().eval()(pixel_values=torch.from_numpy(pixels[:4])).image_embeds.numpy()
    _close(cr.clip_forward(pixels[:4], w, S2, torch.float64)[1], e, "from_pretrained(saved).image_embeds")


def test_directory_saved_by_the_live_clip_vision_model_is_read(tmp_path, pixels):
    """CLIPVisionModel.save_pretrained writes the tower's keys without the "vision_model." prefix (transformers 5)."""
    pytest.importorskip("transformers")
    seed, geom = mk.CASES["B2"]
    small = dataclasses.replace(geom, hidden_size=384, num_heads=6, intermediate_size=256, num_layers=1)
    w = make_clip_weights(seed, small)
    model = mk.hf_model(small, w)
    model.save_pretrained(str(tmp_path))
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.geometry == small and ck.geometry.projection_dim is None and ck.dtype == "float32"
    assert list(ck.tensors) == [n for n, _, _ in clip_tensor_specs(small)]
    assert all(np.array_equal(ck.tensors[k].numpy(), w[k]) for k in w)
    # and the projection class, whose keys carry the prefix
    proj = dataclasses.replace(small, projection_dim=128)
    wp = make_clip_weights(seed, proj)
    pdir = os.path.join(tmp_path, "proj")
    mk.hf_model(proj, wp).save_pretrained(pdir)
    ck = ckpt.read_checkpoint(pdir, "clip")
    assert ck.geometry == proj and all(np.array_equal(ck.tensors[k].numpy(), wp[k]) for k in wp)


def _rewrite_config(path, fn):
    p = os.path.join(path, "config.json")
    cfg = json.load(open(p))
    cfg = fn(cfg) or cfg
    json.dump(cfg, open(p, "w"))


def test_nested_vision_config_and_text_keys_are_accepted(tmp_path):
    from safetensors.torch import load_file, save_file

    w = make_clip_weights(6, S2)
    ckpt.save_checkpoint(tmp_path, w, "clip", "float32", geometry=S2)

    def nest(cfg):
        vc = {k: v for k, v in cfg.items() if k not in ("projection_dim", "architectures")}
        return {"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": cfg["projection_dim"], "logit_scale_init_value": 2.6592,
                "text_config": {"hidden_size": 512, "hidden_act": "gelu_pytorch_tanh", "image_size": 1}, "vision_config": vc}

    _rewrite_config(tmp_path, nest)
    st = os.path.join(tmp_path, "model.safetensors")
    sd = load_file(st)
    sd.update({"text_model.embeddings.token_embedding.weight": torch.zeros(8, 4), "text_model.embeddings.position_ids": torch.zeros(1, 8, dtype=torch.int64),
               "vision_model.embeddings.position_ids": torch.zeros(1, 197, dtype=torch.int64), "text_projection.weight": torch.zeros(4, 4),
               "logit_scale": torch.tensor(2.6592)})
    save_file(sd, st)
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.geometry == S2 and len(ck.tensors) == len(w) and ck.dtype == "float32"
    assert all(np.array_equal(ck.tensors[k].numpy(), w[k]) for k in w)
    # a CLIPVisionModel checkpoint: no visual_projection -> no projection_dim, whatever config.json says
    sd = {k: v for k, v in sd.items() if k != "visual_projection.weight"}
    save_file(sd, st)
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.geometry == dataclasses.replace(S2, projection_dim=None) and ck.geometry.embed_dim == 384 and len(ck.tensors) == len(w) - 1


REFUSALS = [
    ("patch 14", lambda c: c.update(patch_size=14), r"patch_size = 14; supported: 16"),
    ("image 336", lambda c: c.update(image_size=336), r"image_size = 336; supported: 224"),
    ("hidden 512", lambda c: c.update(hidden_size=512, num_attention_heads=8), r"hidden_size = 512; supported: 384, 768, 1024"),
    ("heads of 80", lambda c: c.update(hidden_size=1024, num_attention_heads=1024 // 80), r"num_attention_heads = 12; supported: 16 at hidden_size 1024 \(heads of 64\)"),
    ("tanh GELU", lambda c: c.update(hidden_act="gelu_pytorch_tanh"), r"hidden_act = 'gelu_pytorch_tanh'; supported: gelu, quick_gelu"),
    ("projection 100", lambda c: c.update(projection_dim=100), r"projection_dim = 100; supported: absent, or a multiple of 64 up to 1024"),
    ("projection 1088", lambda c: c.update(projection_dim=1088), r"projection_dim = 1088; supported: absent, or a multiple of 64 up to 1024"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_every_refusal_names_its_field(tmp_path, case):
    _, change, pattern = case
    ckpt.save_checkpoint(tmp_path, make_clip_weights(7, S2), "clip", "float32", geometry=S2)
    _rewrite_config(tmp_path, change)
    with pytest.raises(MmeError, match=pattern):
        ckpt.read_checkpoint(tmp_path, "clip")


def test_missing_and_misshapen_tensors_are_refused(tmp_path):
    w = make_clip_weights(7, S2)
    ckpt.save_checkpoint(tmp_path, {k: v for k, v in w.items() if k != "vision_model.pre_layrnorm.weight"}, "clip", "float32", geometry=S2)
    with pytest.raises(MmeError, match=r"tensor 'vision_model.pre_layrnorm.weight' is missing"):
        ckpt.read_checkpoint(tmp_path, "clip")
    bad = dict(w)
    bad["visual_projection.weight"] = np.zeros((128, 384), dtype=np.float32)
    ckpt.save_checkpoint(tmp_path, bad, "clip", "float32", geometry=S2)
    with pytest.raises(MmeError, match=r"'visual_projection.weight' has shape \(128, 384\), expected \(256, 384\)"):
        ckpt.read_checkpoint(tmp_path, "clip")
    # a CLIP directory read as a ViT: its tensor names are not the ViT's
    ckpt.save_checkpoint(tmp_path, w, "clip", "float32", geometry=S2)
    with pytest.raises(MmeError, match=r"tensor 'embeddings.cls_token' is missing"):
        ckpt.read_checkpoint(tmp_path, "vit")


def test_resample_3_is_accepted_for_clip_only(tmp_path, caplog):
    w = make_clip_weights(7, S2)
    ckpt.save_checkpoint(tmp_path, w, "clip", "float32", geometry=S2, image_mean=(0.48145466, 0.4578275, 0.40821073),
                         image_std=(0.26862954, 0.26130258, 0.27577711), image_processor_type="CLIPImageProcessor")
    p = os.path.join(tmp_path, "preprocessor_config.json")
    pc = json.load(open(p))
    pc.update({"resample": 3, "do_resize": True, "size": {"shortest_edge": 224}, "do_center_crop": True, "crop_size": {"height": 224, "width": 224}})
    json.dump(pc, open(p, "w"))
    ckpt._warned_resize_rule = False
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.image_mean == (0.48145466, 0.4578275, 0.40821073)
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "resample = 3" in text and "do_center_crop" in text and "crop_size" in text and "not applied" in text, text
    pc["resample"] = 1  # anything but BILINEAR / BICUBIC is still refused
    json.dump(pc, open(p, "w"))
    with pytest.raises(MmeError, match=r"resample = 1"):
        ckpt.read_checkpoint(tmp_path, "clip")
    # "vit" refuses resample 3 exactly as before
    vdir = os.path.join(tmp_path, "vit")
    from multimodal_embeddings_amd.weights import VIT_S16

    g = dataclasses.replace(VIT_S16, num_layers=1)
    ckpt.save_checkpoint(vdir, make_vit_weights(1, g), "vit", "float32", geometry=g, image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5))
    vp = os.path.join(vdir, "preprocessor_config.json")
    vpc = json.load(open(vp))
    vpc["resample"] = 3
    json.dump(vpc, open(vp, "w"))
    with pytest.raises(MmeError, match=r"resample = 3; K1 resizes with Pillow BILINEAR \(resample = 2\) only"):
        ckpt.read_checkpoint(vdir, "vit")


def test_both_resize_rules_are_the_identity_on_a_224_input():
    """K1's rule (Mllama fit, Pillow BILINEAR, zero pad) and CLIP's (shortest edge 224 BICUBIC, centre crop 224) on a 224 x 224
    image: neither resamples, so the pixel values are the input's, normalised."""
    from PIL import Image

    from multimodal_embeddings_amd.weights import synthetic_crops
    from oracle import preprocess as opre

    a = synthetic_crops(1, seed=5)[0]
    assert opre.fit_to_canvas(224, 224) == (224, 224)
    clip_rule = np.asarray(Image.fromarray(a).resize((224, 224), Image.BICUBIC))  # shortest edge 224 -> 224 x 224; centre crop 224: all of it
    assert np.array_equal(clip_rule, a)
    pv = opre.preprocess_crop(a)
    lut = opre.normalise_lut()
    assert np.array_equal(pv, np.stack([lut[c][a[:, :, c]] for c in range(3)]))


def test_embedder_names_clip_in_its_refusal():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(ValueError, match="'clip'"):
        RegionEmbedder(encoder="siglip")
