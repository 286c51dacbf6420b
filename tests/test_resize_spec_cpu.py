"""A checkpoint's own preprocessing without a device: the numpy restatement of tests/resize_spec_reference.py against live
Pillow, the recorded hashes and transformers' Pillow processors (ViT, SigLIP with both filters, Bit as DINOv2 configures it,
DeiT's 256 -> 224); the coefficient ranges that keep the kernels' signed 32-bit sums exact; checkpoint.resize_spec_of's
acceptance and refusals; the argument refusals of RegionEmbedder; the ABI lines."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import resize_spec_reference as rsr  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, Engine, MmeError, ResizeSpec  # noqa: E402
from multimodal_embeddings_amd.weights import make_siglip_weights  # noqa: E402
from oracle.preprocess import normalise_lut  # noqa: E402

FIXTURE = json.load(open(os.path.join(HERE, "golden", "resize_spec_cases.json")))
CASES = rsr.case_list()
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def window_of(key, case):
    name, kind, h, w, seed = case
    return rsr.restated_window(key, name, rsr.case_image(name, kind, h, w, seed))


def test_the_fixture_holds_every_spec_and_every_case():
    assert [(c["name"], c["kind"], c["h"], c["w"], c["seed"]) for c in FIXTURE["cases"]] == CASES
    assert len(CASES) == 2 * len(rsr.SHAPES) == 42
    assert set(FIXTURE["specs"]) == set(rsr.SPECS) and len(rsr.SPECS) == 4
    for key, spec in rsr.SPECS.items():
        rec = FIXTURE["specs"][key]
        assert ResizeSpec(**rec["spec"]) == spec and set(rec["windows"]) == {c[0] for c in CASES}


@pytest.mark.parametrize("key", list(rsr.SPECS))
def test_restatement_reproduces_pillow_and_the_fixture(key):
    try:  # the recorded hashes hold where Pillow is absent
        from PIL import Image
    except ImportError:
        Image = None

    spec = rsr.SPECS[key]
    for case in CASES:  # no case is left out: the largest resized image of the list is under 15 MP
        name, kind, h, w, seed = case
        rec = FIXTURE["specs"][key]["windows"][name]
        assert list(rsr.spec_geometry(spec, h, w)) == rec["geometry"]
        new_h, new_w, top, left = rec["geometry"]
        assert 0 <= top <= new_h - 224 and 0 <= left <= new_w - 224 and new_h * new_w < 15_000_000
        win = window_of(key, case)
        assert win.shape == (224, 224, 3) and win.dtype == np.uint8
        assert sha(win) == rec["window_sha256"], f"{key} {name}: the restatement differs from the window Pillow produced when the fixture was made"
        if Image is None:
            continue
        img = rsr.case_image(name, kind, h, w, seed)
        live = np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.Resampling(spec.resample)))[top : top + 224, left : left + 224]
        assert np.array_equal(live, win), f"{key} {name}: live Pillow differs from the restatement in {int((live != win).sum())} bytes"


def processors():
    from transformers import BitImageProcessorPil, DeiTImageProcessorPil, SiglipImageProcessorPil, ViTImageProcessorPil

    return {
        "vit": ("exact224_bilinear", HALF, ViTImageProcessorPil()),
        "siglip_bicubic": ("exact224_bicubic", HALF, SiglipImageProcessorPil()),
        "siglip_bilinear": ("exact224_bilinear", HALF, SiglipImageProcessorPil(resample=2)),
        "bit_dinov2": ("edge256_bicubic", IMAGENET, BitImageProcessorPil(size={"shortest_edge": 256}, resample=3, do_center_crop=True,
                                                                          crop_size={"height": 224, "width": 224}, image_mean=list(IMAGENET[0]),
                                                                          image_std=list(IMAGENET[1]))),
        "deit_256_to_224": ("exact256_bicubic", HALF, DeiTImageProcessorPil(size={"height": 256, "width": 256}, resample=3, do_center_crop=True,
                                                                              crop_size={"height": 224, "width": 224}, image_mean=list(HALF[0]),
                                                                              image_std=list(HALF[1]))),
    }


@pytest.mark.parametrize("which", ["vit", "siglip_bicubic", "siglip_bilinear", "bit_dinov2", "deit_256_to_224"])
def test_restated_pixels_are_what_transformers_feeds_the_tower(which):
    """1e-6 = four f32 ulps at the largest normalised magnitude, 2.64."""
    try:
        from PIL import Image

        key, (mean, std), proc = processors()[which]
    except ImportError:  # as tests/test_clip_preprocess_cpu.py: the comparison runs where Pillow and transformers import
        return
    lut = normalise_lut(mean, std)
    worst = 0.0
    for case in CASES:
        name, kind, h, w, seed = case
        img = rsr.case_image(name, kind, h, w, seed)
        pv = np.asarray(proc(images=[Image.fromarray(img)], return_tensors="np")["pixel_values"][0], dtype=np.float32)
        assert pv.shape == (3, 224, 224)
        win = window_of(key, case)
        ours = np.stack([lut[c][win[:, :, c]] for c in range(3)])
        err = float(np.abs(ours.astype(np.float64) - pv.astype(np.float64)).max())
        worst = max(worst, err)
        assert err <= 1e-6, (which, name, err)
    print(f"{which}: max |restatement + normalise - transformers| = {worst:.3g} over {len(CASES)} cases")


def test_coefficient_ranges_keep_the_signed_sums_exact():
    """|k| < 2^23 (a signed 24-bit multiply is exact), 255 * sum |k| + 2^21 < 2^31, at most 145 taps (the kernels hold 160)."""
    worst = {"max_coeff": 0, "max_abs_sum": 0, "max_taps": 0}
    for key, spec in rsr.SPECS.items():
        for h, w in rsr.SHAPES:
            r = rsr.tap_ranges(spec, h, w)
            worst = {k: max(worst[k], r[k]) for k in worst}
            if spec.resample == 2:
                assert r["max_taps"] <= 73
    print(worst, worst["max_abs_sum"] / (1 << 22))
    assert worst["max_coeff"] < 1 << 23
    assert 255 * worst["max_abs_sum"] + (1 << 21) < 1 << 31
    assert worst["max_taps"] <= 145


# ---- checkpoint.resize_spec_of ------------------------------------------------------------------------------------------
BASE = {"do_rescale": True, "rescale_factor": 1.0 / 255.0, "do_normalize": True, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5]}
VIT_PC = {**BASE, "image_processor_type": "ViTImageProcessor", "do_resize": True, "size": {"height": 224, "width": 224}, "resample": 2}
SIGLIP_PC = {**BASE, "image_processor_type": "SiglipImageProcessor", "do_resize": True, "size": {"height": 224, "width": 224}, "resample": 3}
DINOV2_PC = {**BASE, "image_processor_type": "BitImageProcessor", "do_resize": True, "size": {"shortest_edge": 256}, "resample": 3, "do_center_crop": True,
             "crop_size": {"height": 224, "width": 224}, "do_convert_rgb": True, "image_mean": list(IMAGENET[0]), "image_std": list(IMAGENET[1])}
DEIT_PC = {**BASE, "image_processor_type": "DeiTImageProcessor", "size": {"height": 256, "width": 256}, "resample": 3, "do_center_crop": True, "crop_size": 224}
CLIP_PC = {**BASE, "image_processor_type": "CLIPImageProcessor", "size": 224, "resample": 3, "do_center_crop": True, "crop_size": 224}


@pytest.mark.parametrize("pc, want", [
    (VIT_PC, rsr.SPECS["exact224_bilinear"]),
    (SIGLIP_PC, rsr.SPECS["exact224_bicubic"]),
    ({**SIGLIP_PC, "image_processor_type": "Siglip2ImageProcessor", "resample": 2}, rsr.SPECS["exact224_bilinear"]),
    ({**SIGLIP_PC, "do_center_crop": True, "crop_size": {"height": 224, "width": 224}}, rsr.SPECS["exact224_bicubic"]),
    (DINOV2_PC, rsr.SPECS["edge256_bicubic"]),
    (DEIT_PC, rsr.SPECS["exact256_bicubic"]),
    (CLIP_PC, ResizeSpec("shortest_edge", 224, 0, 3)),
    ({k: v for k, v in VIT_PC.items() if k not in ("do_resize", "do_rescale", "rescale_factor")}, rsr.SPECS["exact224_bilinear"]),
    ({**DINOV2_PC, "do_pad": False}, rsr.SPECS["edge256_bicubic"]),
], ids=["vit", "siglip", "siglip2_fixed_bilinear", "siglip_crop_of_the_whole", "dinov2", "deit", "clip_bare_ints", "defaults_left_out", "do_pad_false"])
def test_resize_spec_of_accepts_what_real_directories_hold(pc, want):
    assert ckpt.resize_spec_of(pc, "preprocessor_config.json") == want


@pytest.mark.parametrize("changes, match", [
    ({"do_center_crop": False}, r"do_center_crop = False with size = \{'shortest_edge': 256\}.*do_center_crop = True with crop_size 224 x 224"),
    ({"do_center_crop": ...}, r"do_center_crop = None with size = \{'shortest_edge': 256\}.*do_center_crop = True"),
    ({"crop_size": {"height": 256, "width": 256}}, r"crop_size = \{'height': 256, 'width': 256\}; supported 224 x 224"),
    ({"crop_size": 336}, r"crop_size = 336; supported 224 x 224"),
    ({"do_pad": True}, r"do_pad = True; supported: no padding"),
    ({"rescale_factor": 1.0 / 127.5}, r"rescale_factor = 0\.0078\d*; supported 1/255"),
    ({"do_rescale": False}, r"do_rescale = False.*supported: do_rescale = True"),
    ({"do_resize": False}, r"do_resize = False.*supported: do_resize = True"),
    ({"resample": 0}, r"resample = 0; supported 2 \(Pillow BILINEAR\) and 3 \(Pillow BICUBIC\)"),
    ({"resample": 1}, r"resample = 1; supported 2 .* and 3 "),
    ({"resample": 4}, r"resample = 4; supported 2 .* and 3 "),
    ({"resample": 5}, r"resample = 5; supported 2 .* and 3 "),
    ({"resample": ...}, r"resample = None; supported 2 .* and 3 "),
    ({"size": {"shortest_edge": 223}}, r"size = \{'shortest_edge': 223\}; supported .*224\.\.512"),
    ({"size": {"shortest_edge": 513}}, r"size = \{'shortest_edge': 513\}; supported .*224\.\.512"),
    ({"size": {"height": 224, "width": 600}}, r"size = \{'height': 224, 'width': 600\}; supported .*224\.\.512"),
    ({"size": {"longest_edge": 224}}, r"size = \{'longest_edge': 224\}; supported \{'shortest_edge': S\}"),
    ({"size": ...}, r"size = None; supported"),
    ({"image_processor_type": "MllamaImageProcessor"}, r"image_processor_type = 'MllamaImageProcessor'.*encoder='mllama_tiles'"),
    ({"image_processor_type": "Siglip2ImageProcessor", "max_num_patches": 256}, r"max_num_patches = 256.*NaFlex.*supported fixed-resolution"),
], ids=lambda v: "-".join(f"{k}={'absent' if x is ... else x}" for k, x in v.items())[:60] if isinstance(v, dict) else "")
def test_resize_spec_of_names_field_value_and_supported_set(changes, match):
    pc = dict(DINOV2_PC)
    for k, v in changes.items():
        if v is ...:
            pc.pop(k, None)
        else:
            pc[k] = v
    with pytest.raises(MmeError, match=match):
        ckpt.resize_spec_of(pc, "preprocessor_config.json")


def test_an_exact_target_other_than_the_canvas_needs_the_centre_crop():
    pc = {k: v for k, v in DEIT_PC.items() if k not in ("do_center_crop", "crop_size")}
    with pytest.raises(MmeError, match=r"do_center_crop = None with size = \{'height': 256, 'width': 256\}.*supported size 224 x 224, or do_center_crop = True"):
        ckpt.resize_spec_of(pc, "preprocessor_config.json")


# ---- a directory, the command line and RegionEmbedder's arguments ------------------------------------------------------------
@pytest.fixture(scope="module")
def siglip_dir(tmp_path_factory):
    import dataclasses

    from multimodal_embeddings_amd.weights import SIGLIP_B16

    geom = dataclasses.replace(SIGLIP_B16, num_layers=1)
    d = tmp_path_factory.mktemp("siglipdir")
    ckpt.save_checkpoint(d, make_siglip_weights(3, geom), "siglip", "float32", geometry=geom, image_mean=HALF[0], image_std=HALF[1],
                         image_processor_type="SiglipImageProcessor")
    return str(d)


def write_pc(d, pc):
    with open(os.path.join(d, "preprocessor_config.json"), "w") as fh:
        json.dump(pc, fh)


def test_read_checkpoint_derives_the_spec_and_refuses_before_loading(siglip_dir, caplog):
    import logging

    write_pc(siglip_dir, SIGLIP_PC)
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(siglip_dir, "siglip", resize_rule="checkpoint")
    assert ck.resize_spec == rsr.SPECS["exact224_bicubic"] and ck.image_mean == HALF[0]
    assert not caplog.records, [r.getMessage() for r in caplog.records]  # the model's own rule runs: nothing to warn of
    assert ckpt.read_checkpoint(siglip_dir, "siglip", resize_rule=rsr.SPECS["exact224_bilinear"]).resize_spec is None
    assert ckpt.read_checkpoint(siglip_dir, "siglip").resize_spec is None
    # refused before any tensor is read: the weights file is gone and the message is still the preprocessor's
    write_pc(siglip_dir, {**SIGLIP_PC, "resample": 1})
    moved = os.path.join(siglip_dir, "model.safetensors")
    os.rename(moved, moved + ".away")
    try:
        with pytest.raises(MmeError, match=r"preprocessor_config\.json: resample = 1; supported 2 "):
            ckpt.read_checkpoint(siglip_dir, "siglip", resize_rule="checkpoint")
        os.remove(os.path.join(siglip_dir, "preprocessor_config.json"))
        with pytest.raises(MmeError, match=r"preprocessor_config\.json is missing: resize_rule = 'checkpoint'"):
            ckpt.read_checkpoint(siglip_dir, "siglip", resize_rule="checkpoint")
    finally:
        os.rename(moved + ".away", moved)


def test_checkpoint_command_line_prints_the_spec(siglip_dir, capsys):
    write_pc(siglip_dir, {**SIGLIP_PC, "resample": 2})
    assert ckpt.main([siglip_dir, "--encoder", "siglip_vit", "--resize-rule", "checkpoint"]) == 0
    assert "resize_spec ResizeSpec(mode='exact', height=224, width=224, resample=2)" in capsys.readouterr().out
    write_pc(siglip_dir, {**SIGLIP_PC, "resample": 5})
    assert ckpt.main([siglip_dir, "--encoder", "siglip_vit", "--resize-rule", "checkpoint"]) == 1
    assert "resample = 5; supported 2" in capsys.readouterr().out


def test_embedder_argument_refusals():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    spec = rsr.SPECS["edge256_bicubic"]
    with pytest.raises(MmeError, match=r"'checkpoint'.*single-tile encoders.*'mllama_tiles'"):
        RegionEmbedder(encoder="mllama_tiles", resize_rule="checkpoint")
    with pytest.raises(MmeError, match=r"ResizeSpec\(mode='shortest_edge', height=256, width=0, resample=3\).*'mllama_tiles'"):
        RegionEmbedder(encoder="mllama_tiles", resize_rule=spec)
    with pytest.raises(MmeError, match=r"resize_rule = 'bicubic'.*'fit_pad', 'clip'.*'checkpoint'.*ResizeSpec"):
        RegionEmbedder(encoder="dinov2", resize_rule="bicubic")
    with pytest.raises(MmeError, match=r"resize_rule = 'checkpoint' reads preprocessor_config\.json of a checkpoint directory"):
        RegionEmbedder("no-such-directory", encoder="dinov2", resize_rule="checkpoint")
    for enc in ("vit_b16", "vit", "clip", "siglip", "dinov2"):
        assert ckpt.check_resize_rule(spec, enc) is spec and ckpt.check_resize_rule("checkpoint", enc) == "checkpoint"
    assert ResizeSpec.of("exact", 224, 3) == ResizeSpec("exact", 224, 224, 3) and ResizeSpec.of("exact", (256, 320), 2) == ResizeSpec("exact", 256, 320, 2)
    assert ResizeSpec.of("shortest_edge", 256, 3) == spec
    with pytest.raises(Exception):  # frozen
        spec.height = 1


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(HERE, "..", "include", "mme.h")).read()
    assert "int mme_set_resize_spec(mme_ctx* ctx, const mme_resize_spec* spec);" in header
    assert "int mme_get_resize_spec(mme_ctx* ctx, mme_resize_spec* out);" in header
    assert "typedef struct mme_resize_spec {" in header and "} mme_resize_spec;" in header
    for field in ("int32_t mode;", "int32_t height;", "int32_t width;", "int32_t resample;"):
        assert field in header
    assert "MME_RESIZE_FIT_PAD = 0, MME_RESIZE_CLIP = 1, MME_RESIZE_SPEC = 2" in header
    assert "MME_RESIZE_MODE_SHORTEST_EDGE = 0, MME_RESIZE_MODE_EXACT = 1" in header
    assert "#define MME_ABI_VERSION 2" in header
    assert "mme_set_resize_spec" in EXPORTS and "mme_get_resize_spec" in EXPORTS
    assert len(EXPORTS["mme_set_resize_spec"][1]) == len(EXPORTS["mme_get_resize_spec"][1]) == 2
    # a spec has parameters: it is not one of the names mme_set_resize_rule takes
    assert Engine.RESIZE_RULES == {"fit_pad": 0, "clip": 1}
    assert isinstance(Engine.resize_spec, property) and callable(Engine.set_resize_spec)
