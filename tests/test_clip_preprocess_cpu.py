"""CLIP's own preprocessing (shortest-edge BICUBIC resize + centre crop), the parts that need no GPU:
the numpy restatement of tests/clip_preprocess_reference.py against the recorded Pillow / transformers hashes of
tests/golden/clip_preprocess_cases.json (and against both libraries live where they import), the size / offset rule, the
preprocessor-file acceptance under resize_rule = "clip", the argument refusals and the ABI symbols.
"""
import hashlib
import json
import logging
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import clip_preprocess_reference as cpr  # noqa: E402
import make_clip_golden as mk  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, MmeError  # noqa: E402
from multimodal_embeddings_amd.weights import make_clip_weights  # noqa: E402
from oracle.preprocess import normalise_lut  # noqa: E402

FIXTURE = json.load(open(os.path.join(HERE, "golden", "clip_preprocess_cases.json")))
CASES = FIXTURE["cases"]
S2 = mk.CASES["S2"][1]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def image_of(case, golden_dir):
    if case["kind"] == "bundled":
        return cpr.bundled_crop(golden_dir, case["name"])
    return cpr.case_image(case["kind"], case["h"], case["w"], case["seed"])


def test_the_fixture_holds_every_case_of_the_list():
    names = [c["name"] for c in CASES]
    assert names[: len(cpr.case_list())] == [c[0] for c in cpr.case_list()]
    assert sum(c["kind"] == "bundled" for c in CASES) == 24
    shapes = {(c["h"], c["w"]) for c in CASES if c["kind"] != "bundled"}
    assert shapes == set(cpr.SHAPES) | {cpr.BIG_SHAPE}
    assert [c["name"] for c in CASES if (c["h"], c["w"]) == cpr.BIG_SHAPE] == ["noise_8000x7168"]  # one instance, noise only


@pytest.mark.parametrize("case", CASES, ids=[c["name"][-40:] for c in CASES])
def test_size_and_offset_rule_equals_the_recorded_tuples(case):
    assert list(cpr.clip_resize_geometry(case["h"], case["w"])) == case["geometry"]
    new_h, new_w, top, left = case["geometry"]
    assert min(new_h, new_w) == 224 and 0 <= top <= new_h - 224 and 0 <= left <= new_w - 224  # the window lies inside: no padding


@pytest.mark.parametrize("case", CASES, ids=[c["name"][-40:] for c in CASES])
def test_restatement_reproduces_pillow_and_transformers(case, golden_dir):
    img = image_of(case, golden_dir)
    assert img.shape == (case["h"], case["w"], 3)
    win = cpr.restated_window(case["name"], img)
    assert win.shape == (224, 224, 3) and win.dtype == np.uint8
    assert sha(win) == case["window_sha256"], "the restatement differs from the window Pillow produced when the fixture was made"
    new_h, new_w, top, left = case["geometry"]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        live = np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BICUBIC))[top : top + 224, left : left + 224]
        assert np.array_equal(live, win), f"live Pillow differs from the restatement in {int((live != win).sum())} bytes"
    try:
        from transformers import CLIPImageProcessorPil
    except ImportError:
        CLIPImageProcessorPil = None
    if CLIPImageProcessorPil is not None and Image is not None:
        pv = np.asarray(CLIPImageProcessorPil()(images=[Image.fromarray(img)], return_tensors="np")["pixel_values"][0], dtype=np.float32)
        lut = normalise_lut()
        ours = np.stack([lut[c][win[:, :, c]] for c in range(3)])
        err = float(np.abs(ours - pv).max())
        print(f"{case['name']}: max |restatement + normalise_lut - transformers| = {err:.3g}")
        assert err <= 1e-6
        assert sha(pv) == case["pixel_values_sha256"]


def test_coefficient_ranges_keep_the_signed_sums_exact():
    """|k| < 2^23 (a signed 24-bit multiply is exact), 255 * sum |k| + 2^21 < 2^31, at most 160 taps (the kernels' MAX_TAPS)."""
    worst = {"max_coeff": 0, "max_abs_sum": 0, "max_taps": 0}
    for h, w in cpr.SHAPES + [cpr.BIG_SHAPE, (8000, 8000), (8000, 224), (224, 8000), (1, 8000), (8000, 1), (7999, 225)]:
        r = cpr.tap_ranges(h, w)
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(worst)
    assert worst["max_coeff"] < 1 << 23
    assert 255 * worst["max_abs_sum"] + (1 << 21) < 1 << 31
    assert worst["max_taps"] <= 145 <= 160


# ---- preprocessor_config.json under resize_rule = "clip" ------------------------------------------------------------
CLIP_PC = {"resample": 3, "do_resize": True, "size": {"shortest_edge": 224}, "do_center_crop": True, "crop_size": {"height": 224, "width": 224}}
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("clipdir")
    ckpt.save_checkpoint(d, make_clip_weights(7, S2), "clip", "float32", geometry=S2, image_mean=MEAN, image_std=STD, image_processor_type="CLIPImageProcessor")
    return str(d)


def write_pc(clip_dir, **changes):
    p = os.path.join(clip_dir, "preprocessor_config.json")
    pc = {"image_processor_type": "CLIPImageProcessor", "do_rescale": True, "rescale_factor": 1.0 / 255.0, "do_normalize": True,
          "image_mean": list(MEAN), "image_std": list(STD), **CLIP_PC}
    for k, v in changes.items():
        if v is ...:
            pc.pop(k)
        else:
            pc[k] = v
    json.dump(pc, open(p, "w"))


@pytest.mark.parametrize("changes", [{}, {"size": 224}, {"crop_size": 224}, {"do_center_crop": ...}, {"do_resize": ...},
                                     {"resample": ..., "size": ..., "crop_size": ...}], ids=str)
def test_matching_preprocessor_file_passes_without_a_warning(clip_dir, caplog, changes):
    write_pc(clip_dir, **changes)
    ckpt._warned_resize_rule = False
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(clip_dir, "clip", resize_rule="clip")
    assert ck.image_mean == MEAN and ck.image_std == STD
    assert not caplog.records, [r.getMessage() for r in caplog.records]
    assert ckpt._warned_resize_rule is False


def test_fit_pad_and_none_keep_the_warning(clip_dir, caplog):
    write_pc(clip_dir)
    for rule in (None, "fit_pad"):
        ckpt._warned_resize_rule = False
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
            ckpt.read_checkpoint(clip_dir, "clip", resize_rule=rule)
        assert "not applied" in " ".join(r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("changes, match", [
    ({"resample": 2}, r"resample = 2; resize_rule = 'clip' .*BICUBIC \(resample = 3\)"),
    ({"size": {"shortest_edge": 336}}, r"size = \{'shortest_edge': 336\}.*'shortest_edge': 224"),
    ({"size": {"height": 224, "width": 224}}, r"size = \{'height': 224, 'width': 224\}.*'shortest_edge': 224"),
    ({"size": 256}, r"size = 256.*224"),
    ({"do_resize": False}, r"do_resize = False.*do_resize = True"),
    ({"do_center_crop": False}, r"do_center_crop = False.*do_center_crop = True"),
    ({"crop_size": 336}, r"crop_size = 336.*224 x 224"),
    ({"crop_size": {"height": 224, "width": 336}}, r"crop_size = \{'height': 224, 'width': 336\}.*224 x 224"),
], ids=lambda v: str(v) if isinstance(v, dict) else "")
def test_each_violation_names_field_value_and_supported_value(clip_dir, changes, match):
    write_pc(clip_dir, **changes)
    with pytest.raises(MmeError, match=match):
        ckpt.read_checkpoint(clip_dir, "clip", resize_rule="clip")


def test_directory_without_a_preprocessor_file_gets_clips_defaults(clip_dir, caplog):
    p = os.path.join(clip_dir, "preprocessor_config.json")
    if os.path.exists(p):
        os.remove(p)
    with caplog.at_level(logging.WARNING, logger="multimodal_embeddings_amd"):
        ck = ckpt.read_checkpoint(clip_dir, "clip", resize_rule="clip")
    assert ck.image_mean is None and ck.image_std is None and not caplog.records  # None: the context's defaults, CLIP's mean / std


def test_checkpoint_command_line_takes_the_rule(clip_dir, capsys):
    write_pc(clip_dir, resample=2)
    assert ckpt.main([clip_dir, "--encoder", "clip", "--resize-rule", "clip"]) == 1
    assert "resample = 2" in capsys.readouterr().out
    write_pc(clip_dir)
    assert ckpt.main([clip_dir, "--encoder", "clip", "--resize-rule", "clip"]) == 0


# ---- argument refusals that need no GPU, and the ABI ----------------------------------------------------------------
def test_rule_refusals():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(MmeError, match=r"'clip'.*'mllama_tiles'"):
        RegionEmbedder(encoder="mllama_tiles", resize_rule="clip")
    with pytest.raises(MmeError, match=r"resize_rule = 'bicubic'.*'fit_pad', 'clip'"):
        RegionEmbedder(encoder="clip", resize_rule="bicubic")
    with pytest.raises(MmeError, match=r"'clip'.*'mllama_tiles'"):
        ckpt.read_checkpoint(".", "mllama_tiles", resize_rule="clip")
    for enc in ("vit_b16", "vit", "clip"):
        assert ckpt.check_resize_rule("clip", enc) == "clip" and ckpt.check_resize_rule(None, enc) == "fit_pad"
    assert ckpt.check_resize_rule(None, "mllama_tiles") == ckpt.check_resize_rule("fit_pad", "mllama_tiles") == "fit_pad"


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(HERE, "..", "include", "mme.h")).read()
    assert "int mme_set_resize_rule(mme_ctx* ctx, int rule);" in header
    assert "int mme_resize_rule(mme_ctx* ctx, int32_t* rule);" in header
    assert "MME_RESIZE_FIT_PAD = 0" in header and "MME_RESIZE_CLIP = 1" in header
    assert "#define MME_ABI_VERSION 2" in header
    assert "mme_set_resize_rule" in EXPORTS and "mme_resize_rule" in EXPORTS
    from multimodal_embeddings_amd._lib import Engine

    assert Engine.RESIZE_RULES == {"fit_pad": 0, "clip": 1} and isinstance(Engine.resize_rule, property)
