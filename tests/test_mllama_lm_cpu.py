"""The Mllama language tower without a GPU: the float64 restatement (tests/mllama_lm_reference.py) against
transformers' recorded fp32 rows, the rotary frequencies, the checkpoint's two key spellings, geometry refusals, the ABI, the
embedder's argument handling, and the SHARPNESS of the golden cases: each wrong tower of `mllama_lm_reference.MUTANTS` lies at
least ten times the engine's bound (1 - cos <= 1e-3) away from the golden rows.

The bound of the first test is stated from fp32 rounding, not fitted: transformers runs the tower in fp32 (unit roundoff
u = 2^-24).  A row passes through 3 layers of 8 rounded stages each (two norms, four matrix products with dot lengths up to
K = 1024, a softmax, the activation); a product's error is at most K u relative to |a| . |b|, which for these seeded towers
(weights ~ N(0, 1 / K), unit rows) is about sqrt(K) u = 2^-19 of the row's scale, and a softmax moves by at most its logits'
error.  24 stages of 2^-19, each allowed an amplification of 4 by the stages behind it: 24 * 4 * 2^-19 = 1.8e-4 of the largest
value of the row.  (Measured when the fixture was made: 8e-7 of it.)
"""
import dataclasses
import json
import os

import numpy as np
import pytest

import mllama_lm_reference as R
from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd import weights as W
from multimodal_embeddings_amd._lib import EXPORTS, Engine, MmeError
from multimodal_embeddings_amd.embedder import RegionEmbedder

HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_BOUND = 1e-3  # 1 - cos of a bf16 tower against fp32 transformers


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "mllama_lm_cases.npz"))


_towers = {}


def tower(name):
    if name not in _towers:
        _towers[name] = R.golden_tower(name)
    return _towers[name]


def inputs(z, case):
    vis = z[case + ".vision"] if case + ".vision" in z else None
    return z[case + ".ids"], z[case + ".lengths"], vis, (z[case + ".xmask"] if vis is not None else None)


def one_minus_cos(a, b):
    return 1.0 - np.sum(a * b, -1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def worst_distance(z, mutant):
    """max over every case and every attended row of 1 - cos(restatement under `mutant`, golden row)"""
    worst = 0.0
    for case, name in R.GOLDEN_CASES.items():
        w, g = tower(name)
        ids, lens, vis, xm = inputs(z, case)
        hs = R.forward(w, g, ids, lens, vis, xm, mutant=mutant)
        gold = z[case + ".hidden"].astype(np.float64)
        S = ids.shape[1]
        for b in range(len(ids)):
            if mutant == "last_row_pooled":  # the row a tower that pools S - 1 returns for the row at len - 1
                worst = max(worst, float(one_minus_cos(hs[b, S - 1], gold[b, lens[b] - 1])))
            else:
                worst = max(worst, float(one_minus_cos(hs[b, : lens[b]], gold[b, : lens[b]]).max()))
    return worst


@pytest.mark.parametrize("case", sorted(R.GOLDEN_CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, case):
    w, g = tower(R.GOLDEN_CASES[case])
    ids, lens, vis, xm = inputs(recorded, case)
    hs = R.forward(w, g, ids, lens, vis, xm)
    gold = recorded[case + ".hidden"].astype(np.float64)
    for b in range(len(ids)):
        rows, want = hs[b, : lens[b]], gold[b, : lens[b]]
        err = np.abs(rows - want).max(-1) / np.abs(want).max(-1)
        print(f"{case}[{b}]: max |restatement - transformers| / max |row| = {err.max():.2e}")
        assert err.max() <= 24 * 4 * 2.0**-19


def test_the_cases_cover_what_they_claim(recorded):
    z = recorded
    assert z["bos_first.xmask"][:, 0].tolist() == [0, 0, 0] and z["bos_first.xmask"][:, 1].tolist() == [1, 3, 15]  # the fully masked BOS row; 1, 2, 4 tiles
    assert z["image_first.xmask"][:, 0].tolist() == [1, 3, 15]
    assert z["two_lengths.lengths"].tolist() == [12, 6] and z["text_only.lengths"].tolist() == [5, 40] and "text_only.vision" not in z
    assert z["bos_first.vision"].shape == (3, 4, R.GOLDEN_TOKENS, 64)
    ga, gb = R.GOLDEN_TOWERS["a"][1], R.GOLDEN_TOWERS["b"][1]
    assert ga.cross_layers == (1,) and gb.cross_layers == (0, 2) and gb.num_kv_heads == gb.num_heads and ga.num_heads == 2 * ga.num_kv_heads
    for name in ("a", "b"):  # gates non-zero, norm weights not all one
        w, g = tower(name)
        assert all(float(v[0]) != 0 for k, v in w.items() if k.endswith("_gate")) and np.ptp(w["language_model.norm.weight"]) > 0.5


def test_rope_frequencies_are_transformers(recorded):
    for name in ("a", "b"):
        g = R.GOLDEN_TOWERS[name][1]
        got, want = W.mllama_rope_inv_freq(g), recorded[name + ".inv_freq"]
        # f32 arithmetic on another library's pow: the interpolated band takes eight rounded operations, and the difference
        # original_max / wavelength - low_freq_factor (up to high_freq_factor = 4) carries them into the result: 16 * 2^-24
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=2.0**-20, atol=0)
    g = R.GOLDEN_BASE
    inv, plain = W.mllama_rope_inv_freq(g), W.mllama_rope_inv_freq(dataclasses.replace(g, rope_type="default"))
    kept, divided = np.isclose(inv, plain, rtol=1e-6), np.isclose(inv, plain / g.rope_factor, rtol=1e-6)
    assert kept.any() and divided.any() and (~kept & ~divided).any(), "the golden frequencies fall in all three llama3 bands"
    cos, sin = W.mllama_rope_tables(g)
    assert cos.shape == sin.shape == (128, 64) and np.all(cos[0] == 1) and np.all(sin[0] == 0)
    full = W.mllama_rope_inv_freq(W.MLLAMA_LM_11B)
    assert full[0] == 1.0 and np.isclose(full[-1], (1.0 / 500000.0 ** (126 / 128)) / 8, rtol=1e-5)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_golden_cases_separate_the_wrong_towers(recorded, mutant):
    d = worst_distance(recorded, mutant)
    print(f"{mutant}: max 1 - cos from the golden rows = {d:.3e}")
    assert d >= 10 * ENGINE_BOUND


def test_the_true_tower_is_far_inside_the_bound(recorded):
    assert worst_distance(recorded, None) <= 1e-9


def test_both_key_spellings_canonicalise_to_one_name_set():
    g = R.GOLDEN_BASE
    names = [s[0] for s in W.mllama_lm_tensor_specs(g)]
    new = ["model." + n for n in names]
    old = [("language_model.model." + n[len("language_model."):]) if n.startswith("language_model.") else n for n in names]
    assert [ckpt.canonical_mllama_lm_name(k) for k in new] == names
    assert [ckpt.canonical_mllama_lm_name(k) for k in old] == names
    for other in ("lm_head.weight", "language_model.lm_head.weight", "model.vision_model.class_embedding", "vision_model.patch_embedding.weight"):
        assert ckpt.canonical_mllama_lm_name(other) is None
    assert ckpt.canonical_tile_name("model.language_model.norm.weight") is None  # and the tile tower's reader leaves these alone


def test_defaults_and_specs():
    g = W.MLLAMA_LM_11B
    assert (g.hidden_size, g.num_heads, g.num_kv_heads, g.intermediate_size, g.num_layers, g.vocab_size) == (4096, 32, 8, 14336, 40, 128256)
    assert g.cross_attention_layers == tuple(range(3, 40, 5)) and g.cross_layers == g.cross_attention_layers and g.embed_rows == 128264
    assert (g.rope_type, g.rope_theta, g.rope_factor, g.rope_low_freq_factor, g.rope_high_freq_factor, g.rope_original_max) == ("llama3", 5e5, 8.0, 1.0, 4.0, 8192)
    assert W.mllama_lm_geometry_problem(g) is None
    cut = dataclasses.replace(g, num_layers=2)  # cross indices beyond the cut are tolerated and ignored
    assert cut.cross_layers == () and W.mllama_lm_geometry_problem(cut) is None
    assert not any("cross_attn" in s[0] for s in W.mllama_lm_tensor_specs(cut))
    params = sum(int(np.prod(s[1])) for s in W.mllama_lm_tensor_specs(g))
    assert 9.2e9 < params < 9.4e9  # 40 layers of ~218 M, 0.53 G of embed_tokens, 31 M of projector; lm_head (0.53 G more) is not loaded
    w, gg = tower("a")
    assert W.infer_mllama_lm_geometry(w, rope_original_max=32) == gg


@pytest.mark.parametrize("change,text", [
    (dict(num_heads=3), "hidden_size = 512 at num_heads = 3"), (dict(num_kv_heads=3), "num_kv_heads = 3"), (dict(intermediate_size=1000), "intermediate_size = 1000"),
    (dict(num_layers=65), "num_layers = 65"), (dict(cross_attention_layers=(2, 1)), "cross_attention_layers = (2, 1)"), (dict(vocab_size=1 << 18), "vocab_size = 262144"),
    (dict(vision_output_dim=100), "vision_output_dim = 100"), (dict(hidden_act="gelu"), "hidden_act = 'gelu'"), (dict(rope_type="yarn"), "rope_type = 'yarn'")])
def test_geometry_refusals_name_the_field_the_value_and_the_supported_set(tmp_path, change, text):
    g = dataclasses.replace(R.GOLDEN_BASE, **change)
    bad = W.mllama_lm_geometry_problem(g)
    assert bad and text in bad and "supported" in bad
    cfg = ckpt._mllama_lm_config(g, "float32", {})  # the same refusal from a directory's config.json, before a tensor is read
    if "rope_type" in change:
        cfg["text_config"]["rope_parameters"]["rope_type"] = "yarn"
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(MmeError, match="supported"):
        ckpt.read_checkpoint(str(tmp_path), "mllama_text")


def test_config_of_both_transformers_generations_reads_alike():
    g = R.GOLDEN_BASE
    cfg = ckpt._mllama_lm_config(g, "bfloat16", {})
    assert ckpt._mllama_lm_geometry(cfg, "x")[0] == g
    old = json.loads(json.dumps(cfg))  # transformers 4.4x: rope_scaling + rope_theta beside it
    rope = old["text_config"].pop("rope_parameters")
    old["text_config"]["rope_theta"] = rope.pop("rope_theta")
    old["text_config"]["rope_scaling"] = rope
    assert ckpt._mllama_lm_geometry(old, "x")[0] == g
    with pytest.raises(MmeError, match="text_config is missing"):
        ckpt._mllama_lm_geometry({"hidden_size": 512}, "x")


def test_a_saved_directory_is_read_back_in_either_spelling(tmp_path):
    import torch
    from safetensors.torch import save_file

    w, g = tower("a")
    d = ckpt.save_checkpoint(str(tmp_path / "new"), w, "mllama_text", "bfloat16", geometry=g)
    ck = ckpt.read_checkpoint(d, "mllama_text")
    assert ck.encoder == "mllama_text" and ck.geometry == g and ck.dtype == "bfloat16" and ck.image_mean is None
    assert set(ck.tensors) == set(w) and all(np.array_equal(ck.tensors[k].float().numpy(), w[k]) for k in w)  # the seeded values are bf16 values
    os.makedirs(tmp_path / "old")
    (tmp_path / "old" / "config.json").write_text((tmp_path / "new" / "config.json").read_text())
    sd = {("language_model.model." + k[len("language_model."):] if k.startswith("language_model.") else k): torch.from_numpy(v).to(torch.bfloat16) for k, v in w.items()}
    sd["language_model.lm_head.weight"] = torch.zeros(8, 512, dtype=torch.bfloat16)
    sd["vision_model.class_embedding"] = torch.zeros(32, dtype=torch.bfloat16)
    save_file(sd, str(tmp_path / "old" / "model.safetensors"))
    ck2 = ckpt.read_checkpoint(str(tmp_path / "old"), "mllama_text")
    assert set(ck2.tensors) == set(w) and all(torch.equal(ck2.tensors[k], ck.tensors[k]) for k in w)
    assert ckpt.main([d, "--encoder", "mllama_text"]) == 0


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(HERE, "..", "include", "mme.h")).read()
    for decl in ("int mme_load_mllama_lm(mme_ctx* ctx, const mme_mllama_lm_weights* w);",
                 "int mme_load_mllama_lm_as(mme_ctx* ctx, const mme_mllama_lm_weights* w, int dtype, void* stream);",
                 "int mme_mllama_lm_info(mme_ctx* ctx, int32_t out[12]);", "int mme_mllama_lm_forward(mme_ctx* ctx, const int32_t* ids_host, const int32_t* len_host,",
                 "int mme_mllama_embed(mme_ctx* ctx, const float* pixel_values_dev,", "int mme_mllama_apply(mme_ctx* ctx, int op, const mme_mllama_apply_args* args, void* stream);",
                 "} mme_mllama_lm_weights;", "} mme_mllama_lm_layer;", "#define MME_ABI_VERSION 2"):
        assert decl in header, decl
    for name in ("mme_load_mllama_lm", "mme_load_mllama_lm_as", "mme_mllama_lm_info", "mme_mllama_lm_forward", "mme_mllama_embed", "mme_mllama_apply"):
        assert name in EXPORTS
    for attr in ("load_mllama_lm", "load_mllama_lm_checkpoint", "mllama_lm_info", "mllama_lm_forward", "mllama_embed", "mllama_apply"):
        assert callable(getattr(Engine, attr))
    assert Engine.MLLAMA_OPS == {"gather": 0, "rmsnorm": 1, "headnorm": 2, "rope": 3, "silu_mul": 4, "pool": 5, "self_attn": 6, "cross_attn": 7}
    assert "mllama_text" in ckpt.ENCODERS and "mllama_text" in ckpt.CLI_ENCODERS
    from multimodal_embeddings_amd import build

    assert {"mllama_lm.hip", "capi_mllama.hip"} <= set(build.SOURCES) and "mllama_lm.h" in build.HEADERS
    import ctypes

    from multimodal_embeddings_amd._lib import _MllamaApplyArgs, _MllamaLMLayer, _MllamaLMWeights

    assert ctypes.sizeof(_MllamaLMLayer) == 16 + 11 * 8 and ctypes.sizeof(_MllamaLMWeights) == 16 * 4 + 5 * 8 and ctypes.sizeof(_MllamaApplyArgs) == 13 * 8 + 16 + 40


class _FakeEngine:
    device = 0
    tile_features = 2560
    resize_rule, resize_spec = "fit_pad", None
    embed_dim = 2560

    def __init__(self, loaded=True):
        self.loaded, self.seen = loaded, None

    def mllama_lm_info(self):
        return {"loaded": self.loaded, "hidden_size": 512, "vocab_size": 300, "image_token_id": 300}

    def mllama_lm_forward(self, ids, lengths, want_bf16=True):
        import torch

        self.seen = (np.array(ids), np.array(lengths))
        return torch.ones((len(ids), 512)) / 512**0.5, None


def test_encoder_mllama_argument_handling():
    with pytest.raises(ValueError, match="belong to encoder='mllama'"):
        RegionEmbedder(encoder="mllama_tiles", prompt_ids=[1, 2], engine=_FakeEngine())
    with pytest.raises(MmeError, match="holds no language tower"):
        RegionEmbedder(encoder="mllama", engine=_FakeEngine(loaded=False), prompt_ids=[1, 300])
    with pytest.raises(ValueError, match="prompt_ids="):  # the default prompt is a str: it needs a tokenizer
        RegionEmbedder(encoder="mllama", engine=_FakeEngine())
    with pytest.raises(ValueError, match="no image token"):
        RegionEmbedder(encoder="mllama", engine=_FakeEngine(), prompt_ids=[1, 2, 3])
    with pytest.raises(MmeError, match="outside 0..307"):
        RegionEmbedder(encoder="mllama", engine=_FakeEngine(), prompt_ids=[1, 300, 308])
    e = RegionEmbedder(encoder="mllama", engine=_FakeEngine(), prompt_ids=[1, 300, 1, 5])
    assert e.embed_dim == 512 and e.prompt_ids == [1, 300, 1, 5] and e.mllama_lm and e.encoder == "mllama_tiles"
    out = e.get_text_embeddings([[1, 5, 6], [1, 7]])
    ids, lens = e.engine.seen
    assert ids.tolist() == [[1, 5, 6], [1, 7, 0]] and lens.tolist() == [3, 2] and len(out) == 2 and len(out[0]) == 512
    assert len(e.get_text_embeddings([1, 5, 6])) == 512 and e.engine.seen[0].tolist() == [[1, 5, 6]]
    with pytest.raises(ValueError, match="prompt_ids="):
        e.get_text_embeddings("a sentence")
    with pytest.raises(MmeError, match="1..128"):
        e.get_text_embeddings([list(range(1, 130))])
    tok = RegionEmbedder(encoder="mllama", engine=_FakeEngine(), tokenizer=lambda s: [1, 300, 1] + [3 + len(w) for w in s.split()])
    assert tok.prompt_ids[:3] == [1, 300, 1] and len(tok.get_text_embeddings("two words")) == 512 and tok.engine.seen[0].tolist() == [[1, 300, 1, 6, 8]]
    with pytest.raises(MmeError, match="config.json is missing"):  # a directory is read as a checkpoint of both towers, never fetched
        RegionEmbedder(HERE, encoder="mllama")


class _DirEngine(_FakeEngine):
    """Stands in for _lib.Engine where RegionEmbedder makes its own contexts from a checkpoint directory."""

    def __init__(self, device=0):
        super().__init__(loaded=False)
        self.device, self.tile_features = device, 64

    def load_tile_vit_checkpoint(self, ck, geometry=None):
        self.tile = ck

    def load_mllama_lm_checkpoint(self, ck):
        self.loaded, self.lm = True, ck


def test_a_directory_brings_its_tokenizer_for_prompt_and_text_queries(tmp_path, monkeypatch):
    """RegionEmbedder(dir, encoder="mllama"): both readers run on the one directory, and the directory's tokenizer files (local files
    only) turn the default prompt AND later str queries into ids -- construction must not lose the tokenizer it found."""
    import types

    import transformers

    from multimodal_embeddings_amd import embedder as emb_mod

    w, g = tower("a")
    d = ckpt.save_checkpoint(str(tmp_path / "both"), w, "mllama_text", "bfloat16", geometry=g)
    (tmp_path / "both" / "tokenizer.json").write_text("{}")
    real, asked = ckpt.read_checkpoint, []

    def read(path, encoder="vit_b16", resize_rule=None):
        asked.append(encoder)
        if encoder == "mllama_tiles":  # a full-geometry vision tower is too large for a test directory
            return types.SimpleNamespace(encoder=encoder, image_mean=None, image_std=None, resize_spec=None, geometry=None)
        return real(path, encoder, resize_rule)

    class Tok:
        def __call__(self, text):
            return {"input_ids": [1, 300, 1] + [3 + len(x) for x in text.split()] if "<|image|>" in text else [1] + [3 + len(x) for x in text.split()]}

    loaded = []

    def from_pretrained(path, local_files_only=False):
        loaded.append((path, local_files_only))
        return Tok()

    monkeypatch.setattr(ckpt, "read_checkpoint", read)
    monkeypatch.setattr(emb_mod, "Engine", _DirEngine)
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(from_pretrained))
    e = RegionEmbedder(d, encoder="mllama", device=0)
    assert asked == ["mllama_tiles", "mllama_text"] and loaded == [(d, True)]
    assert e.engine.lm.geometry == g and e.embed_dim == 512 and e.prompt_ids[:3] == [1, 300, 1]
    assert len(e.get_text_embeddings("Newspaper headline")) == 512 and e.engine.seen[0].tolist() == [[1, 12, 11]]
    out = e.get_text_embeddings(["a b", "c"])
    assert len(out) == 2 and e.engine.seen[1].tolist() == [3, 2]
    own = RegionEmbedder(d, encoder="mllama", device=0, tokenizer=lambda s: [1, 300, 7])  # the caller's tokenizer wins over the directory's
    assert own.prompt_ids == [1, 300, 7] and loaded == [(d, True)]
