"""Patch-32 image towers (ViT/32 @224: 49 patches of 32 x 32, 50 tokens) without a GPU: the float64 restatement of
tests/clip_reference.py at patch 32 against what transformers' own classes returned (tests/golden/clip32_cases.npz,
tests/golden/make_clip32_golden.py); the retile mapping the device uses between K1's patch-16 matrix and the patch-32
matrix; geometry acceptance and inference for both encoders; the checkpoint writer and reader at patch 32; refusals.

Bound of the restatement.  When the fixture was recorded (transformers 5.15.0, float32, eager attention) the float64
restatement was within max(1 - cos) = 2.31e-13 and max |difference| = 2.6e-6 of the recorded rows over the five recorded
matrices (|value| <= 5.5): the float32 rounding of the model's own arithmetic.  The tests assert 4 x those figures.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import clip_reference as cr  # noqa: E402
import make_clip32_golden as mk32  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, CLIP_B32, SUPPORTED_VIT, VIT_B16, VIT_B32, CLIPGeometry, ViTGeometry,  # noqa: E402
                                               clip_geometry_problem, clip_tensor_specs, infer_clip_geometry, infer_vit_geometry,
                                               make_clip_weights, make_vit_weights, vit_geometry_problem, vit_tensor_specs)

ONE_MINUS_COS = 4 * 2.31e-13
MAX_ABS = 4 * 2.6e-6
S32 = mk32.CASES["S32"][1]


def retile_index():
    """(source row, source column) of every element of one crop's patch-32 matrix [49, 3072] in its patch-16 matrix
    [196, 768], from the mapping as the issue states it:
        destination row PY * 7 + PX, column c * 1024 + KY * 32 + KX
        source row (2 PY + KY / 16) * 14 + (2 PX + KX / 16), column c * 256 + (KY % 16) * 16 + KX % 16"""
    P, col = np.meshgrid(np.arange(49), np.arange(3072), indexing="ij")
    PY, PX = P // 7, P % 7
    c, KY, KX = col // 1024, (col % 1024) // 32, col % 32
    return (2 * PY + KY // 16) * 14 + 2 * PX + KX // 16, c * 256 + (KY % 16) * 16 + KX % 16


def retile_np(p16):
    """[n * 196, 768] -> [n * 49, 3072]"""
    p16 = np.asarray(p16)
    n = p16.shape[0] // 196
    srow, scol = retile_index()
    return p16.reshape(n, 196, 768)[:, srow, scol].reshape(n * 49, 3072)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "clip32_cases.npz"))


@pytest.fixture(scope="module")
def pixels():
    return mk32.pixel_values()


def _close(mine, rec, what):
    omc, err = float(cr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{what}: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (what, omc, err)


@pytest.mark.parametrize("key", list(mk32.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, pixels, key):
    seed, geom = mk32.CASES[key]
    assert geom.patch_size == 32 and geom.seq_len == 50 and geom.patch_dim == 3072
    w = make_clip_weights(seed, geom)
    pooled, proj = cr.clip_forward(pixels, w, geom, torch.float64)
    _close(pooled, recorded[f"{key}.pooler_output"], f"{key}.pooler_output")
    assert (proj is not None) == bool(geom.projection_dim) == (f"{key}.image_embeds" in recorded.files)
    if proj is not None:
        assert proj.shape == (mk32.N_CROPS, geom.projection_dim)
        _close(proj, recorded[f"{key}.image_embeds"], f"{key}.image_embeds")
    # sharpness: the same tower with the position rows of two patches exchanged leaves the bound by two orders of magnitude
    sw = dict(w)
    pos = w["vision_model.embeddings.position_embedding.weight"].copy()
    pos[[1, 49]] = pos[[49, 1]]
    sw["vision_model.embeddings.position_embedding.weight"] = pos
    assert float(cr.one_minus_cos(cr.clip_forward(pixels[:4], sw, geom, torch.float64)[0], recorded[f"{key}.pooler_output"][:4]).max()) > 100 * ONE_MINUS_COS


def test_retile_mapping_takes_the_patch16_matrix_to_the_patch32_matrix(pixels):
    pv = torch.from_numpy(pixels[:3])
    p16 = cr.patchify(pv, 16).numpy().reshape(3 * 196, 768)
    p32 = cr.patchify(pv, 32).numpy().reshape(3 * 49, 3072)
    assert np.array_equal(retile_np(p16), p32)
    # a permutation: every source element is used exactly once, and every 16-element run is contiguous on both sides
    srow, scol = retile_index()
    flat = (srow * 768 + scol).reshape(-1)
    assert np.array_equal(np.sort(flat), np.arange(196 * 768))
    runs = flat.reshape(-1, 16)
    assert np.array_equal(runs, runs[:, :1] + np.arange(16)) and not (runs[:, 0] % 16).any()
    # sharpness: the transposed patch grid is another matrix
    wrong = p16.reshape(3, 14, 14, 768).transpose(0, 2, 1, 3).reshape(3 * 196, 768)
    assert not np.array_equal(retile_np(wrong), p32)


def test_geometries_and_inference_for_both_encoders():
    assert SUPPORTED_VIT["patch_size"] == (16, 32)
    assert (VIT_B32.patch_size, VIT_B32.grid, VIT_B32.num_patches, VIT_B32.seq_len, VIT_B32.patch_dim) == (32, 7, 49, 50, 3072)
    assert (VIT_B32.hidden_size, VIT_B32.num_layers, VIT_B32.num_heads, VIT_B32.intermediate_size) == (768, 12, 12, 3072)
    assert CLIP_B32 == dataclasses.replace(CLIP_B16, patch_size=32)
    assert (CLIP_B32.projection_dim, CLIP_B32.hidden_act, CLIP_B32.embed_dim, CLIP_B32.seq_len) == (512, "quick_gelu", 512, 50)
    assert vit_geometry_problem(VIT_B32) is None and clip_geometry_problem(CLIP_B32) is None
    for hidden, heads in ((384, 6), (768, 12), (1024, 16)):
        g = ViTGeometry(patch_size=32, hidden_size=hidden, num_heads=heads, num_layers=1, intermediate_size=64)
        assert vit_geometry_problem(g) is None
    assert vit_geometry_problem(dataclasses.replace(VIT_B16, patch_size=14)) == ("patch_size", 14, "16, 32")
    assert clip_geometry_problem(dataclasses.replace(CLIP_B16, patch_size=14)) == ("patch_size", 14, "16, 32")
    assert vit_geometry_problem(dataclasses.replace(VIT_B32, image_size=384))[0] == "image_size"
    vg = dataclasses.replace(VIT_B32, num_layers=1, intermediate_size=128)
    vw = make_vit_weights(3, vg)
    shapes = {n: s for n, s, _ in vit_tensor_specs(vg)}
    assert shapes["embeddings.position_embeddings"][-2:] == (50, 768)
    assert int(np.prod(shapes["embeddings.patch_embeddings.projection.weight"])) == 768 * 3072
    assert infer_vit_geometry(vw, eps=vg.layer_norm_eps) == vg
    cg = dataclasses.replace(S32, num_layers=1)
    cw = make_clip_weights(3, cg)
    assert cw["vision_model.embeddings.patch_embedding.weight"].shape == (384, 3, 32, 32)
    assert cw["vision_model.embeddings.position_embedding.weight"].shape == (50, 384)
    assert infer_clip_geometry(cw, hidden_act="gelu") == cg
    assert infer_clip_geometry(make_clip_weights(3, dataclasses.replace(cg, patch_size=16)), hidden_act="gelu").patch_size == 16


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_save_then_read_round_trip_at_patch_32(tmp_path, dtype):
    w = make_clip_weights(5, S32)
    ckpt.save_checkpoint(tmp_path, w, "clip", dtype, geometry=S32, image_mean=(0.48145466, 0.4578275, 0.40821073),
                         image_std=(0.26862954, 0.26130258, 0.27577711), image_processor_type="CLIPImageProcessor")
    assert json.load(open(os.path.join(tmp_path, "config.json")))["patch_size"] == 32
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    assert ck.encoder == "clip" and ck.geometry == S32 and ck.geometry.seq_len == 50 and ck.dtype == dtype
    assert list(ck.tensors) == [n for n, _, _ in clip_tensor_specs(S32)]
    for name, t in ck.tensors.items():
        want = torch.from_numpy(w[name]).to(tdt)
        assert t.dtype == tdt and t.shape == want.shape and torch.equal(t.float(), want.float()), name
    assert ckpt.main([str(tmp_path), "--encoder", "clip"]) == 0  # the offline check passes on a patch-32 directory
    # and a plain ViT
    vg = dataclasses.replace(VIT_B32, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=128)
    vdir = os.path.join(tmp_path, "vit")
    vw = make_vit_weights(2, vg)
    ckpt.save_checkpoint(vdir, vw, "vit", dtype, geometry=vg)
    vk = ckpt.read_checkpoint(vdir, "vit")
    assert vk.geometry == vg and all(torch.equal(vk.tensors[k].float().reshape(-1), torch.from_numpy(vw[k]).to(tdt).float().reshape(-1)) for k in vw)
    assert ckpt.main([vdir, "--encoder", "vit"]) == 0


def test_offline_check_under_the_clip_resize_rule(tmp_path):
    w = make_clip_weights(5, S32)
    ckpt.save_checkpoint(tmp_path, w, "clip", "float32", geometry=S32, image_mean=(0.48145466, 0.4578275, 0.40821073),
                         image_std=(0.26862954, 0.26130258, 0.27577711), image_processor_type="CLIPImageProcessor")
    p = os.path.join(tmp_path, "preprocessor_config.json")
    pc = json.load(open(p))
    pc.update({"resample": 3, "do_resize": True, "size": {"shortest_edge": 224}, "do_center_crop": True, "crop_size": {"height": 224, "width": 224}})
    json.dump(pc, open(p, "w"))
    assert ckpt.main([str(tmp_path), "--encoder", "clip", "--resize-rule", "clip"]) == 0


def _rewrite_config(path, fn):
    p = os.path.join(path, "config.json")
    cfg = json.load(open(p))
    fn(cfg)
    json.dump(cfg, open(p, "w"))


@pytest.mark.parametrize("encoder", ["clip", "vit"])
def test_patch_14_is_refused_and_names_both_supported_sizes(tmp_path, encoder):
    if encoder == "clip":
        ckpt.save_checkpoint(tmp_path, make_clip_weights(7, S32), "clip", "float32", geometry=S32)
    else:
        vg = dataclasses.replace(VIT_B32, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=128)
        ckpt.save_checkpoint(tmp_path, make_vit_weights(7, vg), "vit", "float32", geometry=vg)
    _rewrite_config(tmp_path, lambda c: c.update(patch_size=14))
    with pytest.raises(MmeError, match=r"patch_size = 14; supported: 16, 32"):
        ckpt.read_checkpoint(tmp_path, encoder)


def test_patch_32_config_with_patch_16_tensors_is_refused_naming_the_tensor(tmp_path):
    g16 = dataclasses.replace(S32, patch_size=16)
    ckpt.save_checkpoint(tmp_path, make_clip_weights(7, g16), "clip", "float32", geometry=g16)
    _rewrite_config(tmp_path, lambda c: c.update(patch_size=32))
    with pytest.raises(MmeError, match=r"patch_embedding.weight' has shape \(384, 3, 16, 16\), expected \(384, 3, 32, 32\)|"
                                       r"position_embedding.weight' has shape \(197, 384\), expected \(50, 384\)"):
        ckpt.read_checkpoint(tmp_path, "clip")
    # and the other way round
    ckpt.save_checkpoint(tmp_path, make_clip_weights(7, S32), "clip", "float32", geometry=S32)
    _rewrite_config(tmp_path, lambda c: c.update(patch_size=16))
    with pytest.raises(MmeError, match=r"has shape \((384, 3, 32, 32|50, 384)\), expected"):
        ckpt.read_checkpoint(tmp_path, "clip")
