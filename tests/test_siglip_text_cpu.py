"""CPU tests of the SigLIP text tower's host side: the float64 restatement (tests/siglip_text_reference.py) against what
transformers' SiglipTextModel / SiglipModel returned (tests/golden/siglip_text_cases.npz), the mutants that must fall far
outside the bound, the geometry refusals, the checkpoint reader for both key prefixes and the whole-model form, the pad /
length rules of RegionEmbedder.get_text_embeddings on a stand-in engine, and the ABI symbols.  No GPU.

Bounds: tests/golden/make_siglip_text_golden.py printed, for the float64 restatement against the recorded float32 rows,
max(1 - cos) <= 1.86e-13 and max abs <= 1.67e-6 over the four cases, and max abs 1.02e-6 for logits_per_text; the tests
assert 4 x those figures, as the other towers' CPU tests do.
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_siglip_text_golden as mk  # noqa: E402
import siglip_text_reference as tr  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (SIGLIP_B16, SIGLIP_TEXT_B, SiglipTextGeometry, infer_siglip_text_geometry,  # noqa: E402
                                               make_siglip_text_weights, make_siglip_weights, siglip_text_flops_per_sequence,
                                               siglip_text_geometry_problem, siglip_text_tensor_specs, siglip_token_ids)

ONE_MINUS_COS = 4 * 1.86e-13
MAX_ABS = 4 * 1.67e-6
LOGITS_ABS = 4 * 1.02e-6
T2 = SiglipTextGeometry(hidden_size=512, num_layers=2, num_heads=8, intermediate_size=128, vocab_size=64, projection_size=128)  # a quick tower


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "siglip_text_cases.npz"))


@pytest.fixture(scope="module")
def weights():
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = make_siglip_text_weights(mk.CASES[key][0], mk.CASES[key][1])
        return cache[key]

    return get


@pytest.mark.parametrize("key", list(mk.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, weights, key):
    _, geom, _ = mk.CASES[key]
    ids = recorded[f"{key}.ids"]
    assert np.array_equal(ids, mk.case_ids(key)) and ids.dtype == np.int32 and ids.shape == (16, 64)
    real = [int((row != geom.pad_token_id).sum()) for row in ids]
    assert real == list(mk.LENGTHS) and {1, 2, 31, 32, 33, 62, 63, 64} <= set(real)
    mine = tr.siglip_text_forward(ids, weights(key), geom, torch.float64)
    rec = recorded[f"{key}.pooler_output"]
    assert mine.shape == rec.shape == (mk.N_SEQ, geom.projection_size)
    omc, err = float(tr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{key}.pooler_output: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (key, omc, err)


@pytest.mark.parametrize("mutant", [{"pool_pos": 62}, {"causal": True}, {"head_bias": False}])
def test_mutants_fall_far_outside_the_bound(recorded, weights, mutant):
    """pooling position 62 instead of 63, a causal mask, a head without its bias: each at least 1e6 x the bound away"""
    key = "S2"
    _, geom, _ = mk.CASES[key]
    got = tr.siglip_text_forward(recorded[f"{key}.ids"], weights(key), geom, torch.float64, **mutant)
    rec = recorded[f"{key}.pooler_output"]
    omc = float(tr.one_minus_cos(got, rec).max())
    print(f"{mutant}: max(1 - cos) = {omc:.3g}")
    assert omc > 1e6 * ONE_MINUS_COS and float(np.abs(got - rec).max()) > 100 * MAX_ABS


def test_whole_model_logits(recorded, weights):
    key = mk.WHOLE
    w, geom = weights(key), mk.CASES[key][1]
    unit = tr.siglip_text_embed(recorded[f"{key}.ids"], w, geom, torch.float64)
    img = recorded[f"{key}.image_embeds"]
    assert np.allclose(np.linalg.norm(img.astype(np.float64), axis=1), 1.0, atol=1e-6)
    z = tr.siglip_logits_f64(unit, img, float(w["logit_scale"][0]), float(w["logit_bias"][0]))
    err = float(np.abs(z - recorded[f"{key}.logits_per_text"]).max())
    print(f"{key}.logits_per_text: max abs = {err:.3g} (bound {LOGITS_ABS:.3g})")
    assert err <= LOGITS_ABS
    # the two mutants of the scoring step: no bias, a scale that is not exponentiated
    assert float(np.abs(z - float(w["logit_bias"][0]) - recorded[f"{key}.logits_per_text"]).max()) > 1.0
    z_lin = unit @ img.astype(np.float64).T * float(w["logit_scale"][0]) + float(w["logit_bias"][0])
    assert float(np.abs(z_lin - recorded[f"{key}.logits_per_text"]).max()) > 0.1
    p = tr.sigmoid_f64(np.array([-800.0, -100.0, -1.0, 0.0, 1.0, 100.0, 800.0]))
    assert np.isfinite(p).all() and p[0] == 0.0 and p[3] == 0.5 and p[-1] == 1.0 and abs(p[2] + p[4] - 1.0) < 1e-15


def test_v1_case_reaches_both_ends_of_the_siglip2_vocabulary(recorded):
    ids = recorded["V1.ids"]
    assert mk.CASES["V1"][1].vocab_size == 256000 and ids.min() == 0 and ids.max() == 255999
    assert ids[7, 63] == 255999  # the pooled position holds the last row of the table: the offset 255999 * 512 * 2 bytes


def test_padding_is_attended_and_position_63_is_pooled():
    """unlike CLIP's EOS row, the SigLIP row depends on what follows the real tokens: another pad id moves it"""
    w = make_siglip_text_weights(9, T2)
    ids = siglip_token_ids(2, T2.vocab_size, 1, 3, [5, 40])
    a = tr.siglip_text_embed(ids, w, T2)
    other = np.where(ids == 1, 2, ids)
    b = tr.siglip_text_embed(other, w, T2)
    assert float(tr.one_minus_cos(a, b).min()) > 1e-6
    assert np.allclose(np.linalg.norm(a, axis=1), 1.0, atol=1e-12)


def test_defaults_specs_and_flops():
    g = SIGLIP_TEXT_B
    assert (g.hidden_size, g.num_layers, g.num_heads, g.intermediate_size, g.vocab_size, g.max_position_embeddings, g.pad_token_id) == (
        768, 12, 12, 3072, 32000, 64, 1)
    assert g.projection_size == g.embed_dim == 768 and g.hidden_act == "gelu_pytorch_tanh" and siglip_text_geometry_problem(g) is None
    specs = siglip_text_tensor_specs(T2)
    names = [n for n, _, _ in specs]
    assert names[0] == "text_model.embeddings.token_embedding.weight" and names[1] == "text_model.embeddings.position_embedding.weight"
    assert names[-4:] == ["text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias", "text_model.head.weight", "text_model.head.bias"]
    assert len(names) == 2 + 16 * T2.num_layers + 4 and dict((n, s) for n, s, _ in specs)["text_model.head.weight"] == (128, 512)
    w = make_siglip_text_weights(3, T2)
    assert set(w) == set(names) | {"logit_scale", "logit_bias"} and infer_siglip_text_geometry(w) == T2
    assert "logit_scale" not in make_siglip_text_weights(3, T2, logits=None)
    T, D, F, L = 64, 512, 128, 2
    assert siglip_text_flops_per_sequence(T2) == L * (2 * T * D * (4 * D + 2 * F) + 4 * T * T * D) + 2 * D * 128


@pytest.mark.parametrize("change, field, found", [
    ({"hidden_size": 1152, "num_heads": 16}, "hidden_size", 1152),  # so400m: 1152 / heads of 72
    ({"hidden_size": 384, "num_heads": 6}, "hidden_size", 384),
    ({"max_position_embeddings": 77}, "max_position_embeddings", 77),
    ({"num_heads": 12}, "num_heads", 12),
    ({"intermediate_size": 100}, "intermediate_size", 100),
    ({"intermediate_size": 8256}, "intermediate_size", 8256),
    ({"num_layers": 0}, "num_layers", 0),
    ({"num_layers": 65}, "num_layers", 65),
    ({"vocab_size": 2}, "vocab_size", 2),
    ({"vocab_size": 262145}, "vocab_size", 262145),
    ({"hidden_act": "gelu"}, "hidden_act", "gelu"),
    ({"projection_size": 96}, "projection_size", 96),
    ({"projection_size": 1088}, "projection_size", 1088),
    ({"pad_token_id": 64}, "pad_token_id", 64),
])
def test_geometry_refusals_name_the_field_the_value_and_the_supported_set(tmp_path, change, field, found):
    g = dataclasses.replace(T2, **change)
    bad = siglip_text_geometry_problem(g)
    assert bad is not None and bad[0] == field and bad[1] == found and isinstance(bad[2], str) and bad[2]
    # the same refusal from a directory's config.json, before any tensor is read
    ckpt.save_checkpoint(tmp_path, {}, "siglip_text", geometry=g)
    names = {"num_layers": "num_hidden_layers", "num_heads": "num_attention_heads"}
    with pytest.raises(MmeError, match=f"{names.get(field, field)} = {found!r}; supported: "):
        ckpt.read_checkpoint(tmp_path, "siglip_text")


def test_supported_vocabularies_pass():
    for v in (3, 32000, 256000, 262144):
        assert siglip_text_geometry_problem(dataclasses.replace(T2, vocab_size=v)) is None
    for d in (512, 768, 1024):
        assert siglip_text_geometry_problem(dataclasses.replace(T2, hidden_size=d, num_heads=d // 64)) is None


def _write_whole_model(path, wt: dict, gt: SiglipTextGeometry, wv: dict, gv, dtype=torch.float32, naflex=False):
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    cfg = {"architectures": ["SiglipModel"], "model_type": "siglip2_naflex" if naflex else "siglip",
           "text_config": {"model_type": "siglip_text_model", "vocab_size": gt.vocab_size, "hidden_size": gt.hidden_size, "num_hidden_layers": gt.num_layers,
                           "num_attention_heads": gt.num_heads, "intermediate_size": gt.intermediate_size,
                           "max_position_embeddings": gt.max_position_embeddings, "hidden_act": gt.hidden_act, "layer_norm_eps": gt.layer_norm_eps,
                           "pad_token_id": gt.pad_token_id, "projection_size": gt.projection_size},
           "vision_config": {"model_type": "siglip_vision_model", "image_size": gv.image_size, "patch_size": gv.patch_size, "hidden_size": gv.hidden_size,
                             "num_hidden_layers": gv.num_layers, "num_attention_heads": gv.num_heads, "intermediate_size": gv.intermediate_size,
                             "hidden_act": gv.hidden_act, "layer_norm_eps": gv.layer_norm_eps}}
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    sd = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype).contiguous() for k, v in {**wv, **wt}.items()}
    sd["text_model.embeddings.position_ids"] = torch.arange(64).reshape(1, 64)
    save_file(sd, os.path.join(path, "model.safetensors"), metadata={"format": "pt"})


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_both_key_prefixes_and_the_whole_model_are_read_bit_for_bit(tmp_path, dtype):
    from safetensors.torch import save_file

    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    w = make_siglip_text_weights(5, T2)
    want = {k: torch.from_numpy(v).to(tdt) for k, v in w.items()}
    # "text_model." keys (the text half as a SiglipModel names it), with the two scalars
    d1 = ckpt.save_checkpoint(tmp_path / "prefixed", w, "siglip_text", dtype, geometry=T2)
    c1 = ckpt.read_checkpoint(d1, "siglip_text")
    assert c1.encoder == "siglip_text" and c1.geometry == T2 and c1.dtype == dtype and c1.image_mean is None
    assert set(c1.tensors) == set(w) and all(torch.equal(c1.tensors[k], want[k].reshape(c1.tensors[k].shape)) for k in w)
    # bare keys (SiglipTextModel.save_pretrained): no logit_scale / logit_bias
    d2 = tmp_path / "bare"
    ckpt.save_checkpoint(d2, {}, "siglip_text", dtype, geometry=T2)
    bare = {k[len("text_model."):]: want[k].contiguous() for k in w if k.startswith("text_model.")}
    bare["embeddings.position_ids"] = torch.arange(64).reshape(1, 64)
    save_file(bare, os.path.join(d2, "model.safetensors"), metadata={"format": "pt"})
    c2 = ckpt.read_checkpoint(d2, "siglip_text")
    assert c2.geometry == T2 and set(c2.tensors) == {k for k in w if k.startswith("text_model.")}
    assert all(torch.equal(c2.tensors[k], want[k]) for k in c2.tensors)
    # a whole SiglipModel: text_config / vision_config, both towers' keys in one file
    gv = dataclasses.replace(SIGLIP_B16, hidden_size=384, num_layers=1, num_heads=6, intermediate_size=128)
    wv = make_siglip_weights(6, gv)
    d3 = tmp_path / "whole"
    _write_whole_model(d3, w, T2, wv, gv, tdt)
    c3 = ckpt.read_checkpoint(d3, "siglip_text")
    assert c3.geometry == T2 and set(c3.tensors) == set(w) and all(torch.equal(c3.tensors[k], want[k].reshape(c3.tensors[k].shape)) for k in w)
    assert not any(k.startswith("vision_model.") or k.endswith("position_ids") for k in c3.tensors)
    cv = ckpt.read_checkpoint(d3, "siglip")  # the image reader still drops the text half and the scalars
    assert set(cv.tensors) == set(wv) and cv.geometry == gv
    assert ckpt.main([str(d3), "--encoder", "siglip_text"]) == 0


def test_directories_the_reader_refuses(tmp_path):
    w = make_siglip_text_weights(5, T2)
    gv = dataclasses.replace(SIGLIP_B16, hidden_size=384, num_layers=1, num_heads=6, intermediate_size=128)
    d = ckpt.save_checkpoint(tmp_path / "vision", make_siglip_weights(6, gv), "siglip", geometry=gv)
    with pytest.raises(MmeError, match="holds no text tower"):
        ckpt.read_checkpoint(d, "siglip_text")
    _write_whole_model(tmp_path / "naflex", w, T2, {}, gv, naflex=True)
    with pytest.raises(MmeError, match="NaFlex"):
        ckpt.read_checkpoint(tmp_path / "naflex", "siglip_text")
    one = {k: v for k, v in w.items() if k != "logit_bias"}
    d = ckpt.save_checkpoint(tmp_path / "one_scalar", one, "siglip_text", geometry=T2)
    with pytest.raises(MmeError, match="logit_scale"):
        ckpt.read_checkpoint(d, "siglip_text")
    assert "siglip_text" in ckpt.ENCODERS and "siglip_text" in ckpt.CLI_ENCODERS and "siglip_text" not in ckpt.CLIP_RULE_ENCODERS


# ---- RegionEmbedder's host plumbing, on a stand-in engine ----------------------------------------------------------------
class _FakeEngine:
    def __init__(self, pad=1, dim=8):
        self.pad, self.dim, self.seen = pad, dim, None

    def text_info(self):
        return {"loaded": 1, "eos_token_id": self.pad, "vocab_size": 195, "projection_dim": self.dim, "hidden_size": 512}

    def text_geometry(self):
        return {"kind": "siglip", "tokens": 64, "projection": self.dim, "pad_token_id": self.pad}

    def text_forward(self, ids, want_f32=True, want_bf16=True):
        self.seen = np.array(ids)
        return torch.full((len(ids), self.dim), self.dim ** -0.5), None


def _embedder(tokenizer=None, text_dir=None):
    e = RegionEmbedder.__new__(RegionEmbedder)
    e.engines = [_FakeEngine()]
    e.encoder = "siglip"
    e._text_source, e._text_loaded, e._tokenizer, e._text_dir = True, True, tokenizer, text_dir
    return e


def test_token_ids_are_right_padded_to_64_and_long_ones_refused():
    e = _embedder()
    v = e.get_text_embeddings([5, 6, 7])
    assert isinstance(v, list) and len(v) == 8
    seen = e.engines[0].seen
    assert seen.shape == (1, 64) and seen[0, :3].tolist() == [5, 6, 7] and (seen[0, 3:] == 1).all()
    out = e.get_text_embeddings(np.array([[5, 9, 9], [7, 8, 9]]))
    assert len(out) == 2 and e.engines[0].seen.shape == (2, 64) and e.engines[0].seen[1, :4].tolist() == [7, 8, 9, 1]
    assert len(e.get_text_embeddings([[5], [7, 8, 9, 4]])) == 2 and e.get_text_embeddings([]) == []
    assert len(e.get_text_embeddings(list(range(64)))) == 8 and (e.engines[0].seen[0] == np.arange(64)).all()  # exactly 64: nothing padded
    with pytest.raises(MmeError, match="65 token ids; supported: at most 64"):
        e.get_text_embeddings(list(range(65)))
    with pytest.raises(MmeError, match="1-D integer sequence"):
        e.get_text_embeddings([0.5, 1.5])


def test_strings_go_through_the_tokenizer_padded_to_64(tmp_path):
    e = _embedder(tokenizer=lambda s: [ord(c) for c in s])
    assert len(e.get_text_embeddings("ab")) == 8 and e.engines[0].seen[0, :4].tolist() == [97, 98, 1, 1]

    class Tok:  # a transformers-style tokenizer: called with SigLIP's arguments
        pad_token_id = 1

        def __call__(self, text, padding=None, max_length=None, truncation=None):
            assert (padding, max_length, truncation) == ("max_length", 64, True)
            ids = [ord(c) for c in text][:64]
            return {"input_ids": ids + [1] * (64 - len(ids))}

    e = _embedder(tokenizer=Tok())
    assert len(e.get_text_embeddings(["ab", "c" * 100])) == 2 and e.engines[0].seen.shape == (2, 64) and (e.engines[0].seen[1] == ord("c")).all()
    with pytest.raises(MmeError, match="token ids .* are accepted"):
        _embedder().get_text_embeddings("no tokenizer and no directory")
    with pytest.raises(MmeError, match="token ids .* are accepted"):
        _embedder(text_dir=str(tmp_path)).get_text_embeddings("a directory without tokenizer files")


def test_a_siglip_embedder_without_a_tower_is_still_a_stub():
    e = _embedder()
    e._text_source, e._text_loaded, e.checkpoint = None, False, None
    with pytest.raises(NotImplementedError, match="SigLIP text tower"):
        e.get_text_embeddings([1, 2])
    e._text_source = False
    with pytest.raises(NotImplementedError):
        e.get_text_embeddings([1, 2])
    with pytest.raises(NotImplementedError):
        e.siglip_probabilities([[1, 2]], np.zeros((1, 64), np.float32))


def test_width_mismatch_is_refused_before_any_load():
    e = _embedder()
    e._text_loaded, e.embed_dim = False, 768
    e._text_source = make_siglip_text_weights(3, T2)  # projects to 128
    with pytest.raises(MmeError, match="projection_size = 128; supported: 768"):
        e.get_text_embeddings([1, 2])


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "mme.h")).read()
    for name in ("mme_load_siglip_text", "mme_load_siglip_text_as", "mme_text_geometry", "mme_siglip_scores", "mme_siglip_text_apply"):
        assert name in EXPORTS and f"int {name}(" in header
    assert "#define MME_ABI_VERSION 2" in header and "int mme_text_info(mme_ctx* ctx, int32_t out[9]);" in header
    for m in ("load_siglip_text", "load_siglip_text_checkpoint", "siglip_scores", "siglip_text_apply", "text_geometry"):
        assert callable(getattr(Engine, m))
    assert Engine.SIGLIP_TEXT_OPS == {"token_rows": 0, "attention": 1, "last_pool_ln": 2, "bias_l2": 3, "scores": 4}
