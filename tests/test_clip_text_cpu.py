"""The CLIP text tower without a GPU: the float64 restatement (tests/clip_text_reference.py) against what transformers' own
classes returned (tests/golden/clip_text_cases.npz, tests/golden/make_clip_text_golden.py); the geometry refusals; the
checkpoint directory reader and writer for encoder "clip_text"; the tokenizer and token-id plumbing of
RegionEmbedder.get_text_embeddings; the stub; the ABI symbols; and the float64 proof that the GPU attention cases can tell a
wrong mask, admitted padding and a missing scale from the kernel's contract.

Bound of the restatement.  When the fixture was recorded (transformers 5.15.0, float32, eager attention) the float64
restatement was within max(1 - cos) = 4.12e-13 and max |difference| = 4.14e-6 of the recorded rows over the nine recorded
matrices (|value| <= 5.54): the float32 rounding of the model's own arithmetic.  The tests assert 4 x those figures, the
rule of tests/test_clip_cpu.py.
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

import clip_text_reference as tr  # noqa: E402
import make_clip_text_golden as mk  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, CLIP_TEXT_B, CLIPTextGeometry, clip_text_flops_per_sequence,  # noqa: E402
                                               clip_text_geometry_problem, clip_text_tensor_specs, infer_clip_text_geometry, make_clip_text_weights,
                                               make_clip_weights, round_to_bf16, synthetic_token_ids)

ONE_MINUS_COS = 4 * 4.12e-13
MAX_ABS = 4 * 4.14e-6
T2 = CLIPTextGeometry(num_layers=2, intermediate_size=128, vocab_size=64, eos_token_id=63, projection_dim=128)  # a quick tower


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "clip_text_cases.npz"))


def _close(mine, rec, what):
    omc, err = float(tr.one_minus_cos(mine, rec).max()), float(np.abs(mine - rec.astype(np.float64)).max())
    print(f"{what}: max(1 - cos) = {omc:.3g} (bound {ONE_MINUS_COS:.3g}), max abs = {err:.3g} (bound {MAX_ABS:.3g})")
    assert omc <= ONE_MINUS_COS and err <= MAX_ABS, (what, omc, err)


@pytest.mark.parametrize("key", list(mk.CASES))
def test_restatement_agrees_with_the_recorded_transformers_rows(recorded, key):
    seed, geom, term, _ = mk.CASES[key]
    ids = recorded[f"{key}.ids"]
    assert np.array_equal(ids, mk.case_ids(key)) and ids.dtype == np.int32
    assert np.array_equal(tr.eos_positions(ids, geom.eos_token_id), np.array(mk.LENGTHS) - 1)  # both rules find the terminator
    w = make_clip_text_weights(seed, geom)
    pooled, proj = tr.clip_text_forward(ids, w, geom, torch.float64)
    _close(pooled, recorded[f"{key}.pooler_output"], f"{key}.pooler_output")
    assert (proj is not None) == bool(geom.projection_dim) == (f"{key}.text_embeds" in recorded.files)
    if proj is not None:
        assert proj.shape == (mk.N_SEQ, geom.projection_dim)
        _close(proj, recorded[f"{key}.text_embeds"], f"{key}.text_embeds")
    # sharpness: the other activation, and the row before the EOS pooled, are far outside
    other = dataclasses.replace(geom, hidden_act="gelu" if geom.hidden_act == "quick_gelu" else "quick_gelu")
    assert float(tr.one_minus_cos(tr.clip_text_forward(ids[4:8], w, other, torch.float64)[0], recorded[f"{key}.pooler_output"][4:8]).max()) > 1e-6
    shifted = ids.copy()[4:8]
    for i, n in enumerate(mk.LENGTHS[4:8]):
        shifted[i, n - 2 :] = term  # the terminator one position early
    assert float(tr.one_minus_cos(tr.clip_text_forward(shifted, w, geom, torch.float64)[0], recorded[f"{key}.pooler_output"][4:8]).max()) > 1e-4


def test_v1_case_reaches_both_ends_of_the_real_vocabulary(recorded):
    ids = recorded["V1.ids"]
    assert {0, 49406, 49407} <= set(np.unique(ids).tolist()) and mk.CASES["V1"][1].vocab_size == 49408
    assert mk.CASES["H2"][1].eos_token_id == 2 and int(recorded["H2.ids"].max()) == 1023  # the legacy rule: argmax


def test_eos_row_does_not_depend_on_what_follows_it():
    seed, geom, term, _ = mk.CASES["B2n"]
    w = make_clip_text_weights(seed, geom)
    ids = mk.case_ids("B2n")[[0, 3, 5, 9, 13]]
    zero_pad = ids.copy()
    for i, p in enumerate(tr.eos_positions(ids, geom.eos_token_id)):
        zero_pad[i, p + 1 :] = 0
    a, b = tr.clip_text_forward(ids, w, geom, torch.float64)[0], tr.clip_text_forward(zero_pad, w, geom, torch.float64)[0]
    assert np.array_equal(a, b)  # the causal mask: not one bit of the pooled row moves


def test_eos_rules():
    ids = synthetic_token_ids(3, 64, 63, 7, [2, 40, 77])
    assert ids.shape == (3, 77) and ids.dtype == np.int32 and (ids[0, 1:] == 63).all() and (ids[1, :39] != 63).all() and ids[2, 76] == 63
    assert np.array_equal(tr.eos_positions(ids, 63), [1, 39, 76])
    assert np.array_equal(tr.eos_positions(ids, 2), [1, 39, 76])  # legacy: the largest id is the terminator
    legacy = ids.copy()
    legacy[1, 5] = 63  # an earlier occurrence wins under both rules
    assert tr.eos_positions(legacy, 63)[1] == 5 and tr.eos_positions(legacy, 2)[1] == 5
    none = ids.copy()
    none[1] = 7
    assert tr.eos_positions(none, 63)[1] == -1  # the library refuses such a sequence with its index (tests/test_gpu_clip_text.py)
    with pytest.raises(ValueError):
        synthetic_token_ids(2, 64, 63, 0, [1, 78])


# ---- geometry --------------------------------------------------------------------------------------------------------
def test_defaults_specs_and_flops():
    g = CLIP_TEXT_B
    assert (g.hidden_size, g.num_layers, g.num_heads, g.intermediate_size, g.vocab_size, g.eos_token_id) == (512, 12, 8, 2048, 49408, 49407)
    assert (g.projection_dim, g.hidden_act, g.layer_norm_eps, g.max_position_embeddings, g.embed_dim) == (512, "quick_gelu", 1e-5, 77, 512)
    assert clip_text_geometry_problem(g) is None and all(clip_text_geometry_problem(c[1]) is None for c in mk.CASES.values())
    w = make_clip_text_weights(3, T2)
    assert [n for n, _, _ in clip_text_tensor_specs(T2)] == list(w) and len(w) == 2 + 16 * 2 + 2 + 1
    assert list(w)[0] == "text_model.embeddings.token_embedding.weight" and list(w)[-2:] == ["text_model.final_layer_norm.bias", "text_projection.weight"]
    for name, shape, kind in clip_text_tensor_specs(T2):
        assert w[name].shape == tuple(shape) and np.array_equal(round_to_bf16(w[name]), w[name]), name
        if kind == "gamma":
            assert 0.15 < float(np.abs(w[name] - 1).mean()) < 0.3, name
        if kind == "bias" and "norm" in name:
            assert 0.05 < float(np.abs(w[name]).mean()) < 0.12, name
    assert infer_clip_text_geometry(w) == T2
    assert "text_projection.weight" not in make_clip_text_weights(3, dataclasses.replace(T2, projection_dim=None))
    D, F, L = 512, 2048, 12
    assert clip_text_flops_per_sequence(g) == L * (2 * 77 * D * (4 * D + 2 * F) + 4 * (77 * 78 // 2) * D) + 2 * D * 512


@pytest.mark.parametrize("change, field, found", [
    (dict(hidden_size=640, num_heads=10), "hidden_size", 640),
    (dict(num_heads=12), "num_heads", 12),
    (dict(max_position_embeddings=64), "max_position_embeddings", 64),
    (dict(intermediate_size=100), "intermediate_size", 100),
    (dict(vocab_size=70000), "vocab_size", 70000),
    (dict(projection_dim=96), "projection_dim", 96),
    (dict(hidden_act="gelu_pytorch_tanh"), "hidden_act", "gelu_pytorch_tanh"),
])
def test_geometry_refusals_name_the_field_the_value_and_the_supported_set(tmp_path, change, field, found):
    bad = clip_text_geometry_problem(dataclasses.replace(T2, **change))
    assert bad is not None and bad[0] == field and bad[1] == found and bad[2]
    # and through a checkpoint directory's config.json
    ckpt.save_checkpoint(tmp_path, make_clip_text_weights(1, T2), "clip_text", geometry=T2)
    cfg = json.load(open(tmp_path / "config.json"))
    names = {"hidden_size": "hidden_size", "num_heads": "num_attention_heads", "max_position_embeddings": "max_position_embeddings",
             "intermediate_size": "intermediate_size", "vocab_size": "vocab_size", "projection_dim": "projection_dim", "hidden_act": "hidden_act"}
    for k, v in change.items():
        cfg[names[k]] = v
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    with pytest.raises(MmeError) as e:
        ckpt.read_checkpoint(tmp_path, "clip_text")
    assert f"{names[field]} = {found!r}; supported: " in str(e.value)


# ---- checkpoint directories --------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _write(dirpath, tensors: dict, cfg: dict, dtype):
    from safetensors.torch import save_file

    os.makedirs(dirpath, exist_ok=True)
    json.dump(cfg, open(os.path.join(dirpath, "config.json"), "w"))
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).contiguous() for k, v in tensors.items()}, os.path.join(dirpath, "model.safetensors"),
              metadata={"format": "pt"})


def _text_cfg(g, **extra):
    c = {"vocab_size": g.vocab_size, "hidden_size": g.hidden_size, "num_hidden_layers": g.num_layers, "num_attention_heads": g.num_heads,
         "intermediate_size": g.intermediate_size, "max_position_embeddings": 77, "hidden_act": g.hidden_act, "layer_norm_eps": g.layer_norm_eps,
         "eos_token_id": g.eos_token_id}
    c.update(extra)
    return c


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_the_three_directory_kinds_are_read_bit_for_bit(tmp_path, dtype):
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    w = make_clip_text_weights(5, T2)

    def same(ck, geom):
        assert ck.encoder == "clip_text" and ck.geometry == geom and ck.dtype == dtype and ck.image_mean is None
        assert list(ck.tensors) == [n for n, _, _ in clip_text_tensor_specs(geom)]
        for name, t in ck.tensors.items():
            want = torch.from_numpy(w[name]).to(tdt)
            assert t.dtype == tdt and t.shape == want.shape and torch.equal(_bits(t), _bits(want)), name

    # (1) CLIPTextModelWithProjection, by the project's own writer
    ckpt.save_checkpoint(tmp_path / "proj", w, "clip_text", dtype, geometry=T2)
    same(ckpt.read_checkpoint(tmp_path / "proj", "clip_text"), T2)
    assert ckpt.main([str(tmp_path / "proj"), "--encoder", "clip_text"]) == 0
    # (2) a whole CLIPModel: both towers, both projections, logit_scale, position_ids; projection_dim at the top level
    vg = dataclasses.replace(CLIP_B16, hidden_size=384, num_layers=1, num_heads=6, intermediate_size=64, projection_dim=128)
    vw = make_clip_weights(6, vg)
    whole = dict(w)
    whole.update(vw)
    whole["logit_scale"] = np.float32([2.6592])
    whole["text_model.embeddings.position_ids"] = np.arange(77, dtype=np.float32)[None]
    vcfg = {"image_size": 224, "patch_size": 16, "hidden_size": 384, "num_hidden_layers": 1, "num_attention_heads": 6, "intermediate_size": 64,
            "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}
    _write(tmp_path / "whole", whole, {"model_type": "clip", "projection_dim": 128, "text_config": _text_cfg(T2, projection_dim=512), "vision_config": vcfg}, tdt)
    same(ckpt.read_checkpoint(tmp_path / "whole", "clip_text"), T2)
    # ... and the same directory still reads as "clip" exactly as before: the image tower alone
    ck = ckpt.read_checkpoint(tmp_path / "whole", "clip")
    assert ck.encoder == "clip" and ck.geometry == vg and list(ck.tensors) == list(vw)
    for name, t in ck.tensors.items():
        assert torch.equal(_bits(t), _bits(torch.from_numpy(vw[name]).to(tdt))), name
    # (3) CLIPTextModel: the tower's own keys, no "text_model." prefix, no projection
    g3 = dataclasses.replace(T2, projection_dim=None)
    bare = {k[len("text_model."):]: v for k, v in w.items() if k.startswith("text_model.")}
    _write(tmp_path / "bare", bare, dict(_text_cfg(T2, projection_dim=512), model_type="clip_text_model"), tdt)
    same(ckpt.read_checkpoint(tmp_path / "bare", "clip_text"), g3)
    assert ckpt.canonical_clip_name("text_model.final_layer_norm.weight") is None  # canonical_clip_name is unchanged
    assert ckpt.canonical_clip_text_name("vision_model.post_layernorm.weight") is None and ckpt.canonical_clip_text_name("logit_scale") is None


def test_a_directory_without_a_text_tower_is_refused(tmp_path):
    vg = dataclasses.replace(CLIP_B16, hidden_size=384, num_layers=1, num_heads=6, intermediate_size=64, projection_dim=128)
    ckpt.save_checkpoint(tmp_path, make_clip_weights(6, vg), "clip", geometry=vg)
    with pytest.raises(MmeError):
        ckpt.read_checkpoint(tmp_path, "clip_text")


def test_saved_directory_loads_into_transformers(tmp_path):
    tf = pytest.importorskip("transformers")
    w = make_clip_text_weights(12, T2)
    ckpt.save_checkpoint(tmp_path, w, "clip_text", "float32", geometry=T2)
    model, info = tf.CLIPTextModelWithProjection.from_pretrained(str(tmp_path), output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"] and not info["mismatched_keys"], info
    ids = synthetic_token_ids(4, 64, 63, 1, [2, 33, 64, 77])
    with torch.no_grad():
        e = model.float().eval()(input_ids=torch.from_numpy(ids.astype(np.int64))).text_embeds.numpy()
    _close(tr.clip_text_forward(ids, w, T2, torch.float64)[1], e, "from_pretrained(saved).text_embeds")


# ---- RegionEmbedder's host plumbing, on a stand-in engine ----------------------------------------------------------------
class _FakeEngine:
    def __init__(self, eos=194, dim=8):
        self.eos, self.dim, self.seen = eos, dim, None

    def text_info(self):
        return {"loaded": 1, "eos_token_id": self.eos, "vocab_size": 195, "projection_dim": self.dim, "hidden_size": 512}

    def text_forward(self, ids, want_f32=True, want_bf16=True):
        self.seen = np.array(ids)
        return torch.full((len(ids), self.dim), self.dim ** -0.5), None


def _embedder(tokenizer=None, text_dir=None):
    e = RegionEmbedder.__new__(RegionEmbedder)
    e.engines = [_FakeEngine()]
    e._text_source, e._text_loaded, e._tokenizer, e._text_dir = True, True, tokenizer, text_dir
    return e


def toy_tokenizer_files(d):
    """printable ASCII with and without </w>, five merges, <|startoftext|> and <|endoftext|> as the last two ids (193, 194)"""
    chars = [chr(c) for c in range(33, 127)]
    vocab = {}
    for tok in chars + [c + "</w>" for c in chars] + ["th", "the</w>", "ne", "new", "news</w>", "<|startoftext|>", "<|endoftext|>"]:
        vocab[tok] = len(vocab)
    os.makedirs(d, exist_ok=True)
    json.dump(vocab, open(os.path.join(d, "vocab.json"), "w"))
    open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\nt h\nth e</w>\nn e\nne w\nnew s</w>\n")
    return vocab


def test_token_ids_are_right_padded_and_long_ones_refused():
    e = _embedder()
    v = e.get_text_embeddings([5, 6, 194])
    assert isinstance(v, list) and len(v) == 8 and all(isinstance(x, float) for x in v)
    seen = e.engines[0].seen
    assert seen.shape == (1, 77) and seen[0, :3].tolist() == [5, 6, 194] and (seen[0, 3:] == 194).all()
    assert len(e.get_text_embeddings(np.array([5, 194], dtype=np.int32))) == 8  # a 1-D array is one query
    out = e.get_text_embeddings(np.array([[5, 194, 194], [7, 8, 194]]))  # a 2-D array is a list of queries
    assert len(out) == 2 and len(out[0]) == 8 and e.engines[0].seen[1, :4].tolist() == [7, 8, 194, 194]
    assert len(e.get_text_embeddings([[5, 194], [7, 8, 9, 194]])) == 2 and e.get_text_embeddings([]) == []
    assert len(e.get_text_embeddings(list(range(76)) + [194])) == 8  # exactly 77
    with pytest.raises(MmeError, match="78 token ids; supported: at most 77"):
        e.get_text_embeddings(list(range(77)) + [194])
    with pytest.raises(MmeError, match="1-D integer sequence"):
        e.get_text_embeddings([0.5, 1.5])


def test_strings_go_through_the_tokenizer(tmp_path):
    e = _embedder(tokenizer=lambda s: [ord(c) for c in s] + [194])
    assert len(e.get_text_embeddings("ab")) == 8 and e.engines[0].seen[0, :4].tolist() == [97, 98, 194, 194]
    assert len(e.get_text_embeddings(["ab", "c"])) == 2
    with pytest.raises(MmeError, match="token ids .* are accepted"):
        _embedder().get_text_embeddings("no tokenizer and no directory")
    with pytest.raises(MmeError, match="token ids .* are accepted"):
        _embedder(text_dir=str(tmp_path)).get_text_embeddings("a directory without tokenizer files")


def test_strings_go_through_a_clip_tokenizer_read_from_local_files(tmp_path):
    pytest.importorskip("transformers")
    toy_tokenizer_files(tmp_path / "tok")
    e = _embedder(text_dir=str(tmp_path / "tok"))  # the lazy CLIPTokenizer.from_pretrained(dir, local_files_only=True)
    e.get_text_embeddings("The news")
    assert e.engines[0].seen[0, :5].tolist() == [193, 189, 192, 194, 194] and (e.engines[0].seen[0, 5:] == 194).all()
    e.get_text_embeddings("The news " * 40)
    assert e.engines[0].seen.shape == (1, 77) and e.engines[0].seen[0, 76] == 194 and e.engines[0].seen[0, 0] == 193
    from transformers import CLIPTokenizer

    e2 = _embedder(tokenizer=CLIPTokenizer.from_pretrained(str(tmp_path / "tok"), local_files_only=True))  # a tokenizer object
    e2.get_text_embeddings("news")
    assert e2.engines[0].seen[0, :3].tolist() == [193, 192, 194]


def test_an_embedder_without_a_tower_is_still_a_stub():
    bare = RegionEmbedder.__new__(RegionEmbedder)  # no attribute at all
    with pytest.raises(NotImplementedError):
        bare.get_text_embeddings("Hoosier. Hockey.")
    off = _embedder()
    off._text_source = False
    with pytest.raises(NotImplementedError):
        off.get_text_embeddings([1, 2, 194])


def test_query_without_embeddings_or_texts_raises_as_before():
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    col = RegionCollection.__new__(RegionCollection)
    with pytest.raises(ValueError, match=r"query_embeddings is required \(text queries need the language tower, which is out of scope\)"):
        col.query()
    with pytest.raises(ValueError, match="query_embeddings is required"):
        col.query(query_texts=["a"])  # no embedder to embed them with


def test_abi_symbols_are_declared_and_bound():
    header = open(os.path.join(HERE, "..", "include", "mme.h")).read()
    for decl in ("int mme_load_clip_text(mme_ctx* ctx, const mme_clip_text_weights* w);",
                 "int mme_load_clip_text_as(mme_ctx* ctx, const mme_clip_text_weights* w, int dtype, void* stream);",
                 "int mme_text_info(mme_ctx* ctx, int32_t out[9]);",
                 "int mme_text_forward(mme_ctx* ctx, const int32_t* ids_host, int n, float* emb_f32, uint16_t* emb_bf16, void* stream);",
                 "int mme_text_apply(mme_ctx* ctx, int op, const mme_text_apply_args* args, void* stream);",
                 "} mme_clip_text_weights;", "#define MME_ABI_VERSION 2", "#define MME_TEXT_CHUNK 1024"):
        assert decl in header, decl
    for name in ("mme_load_clip_text", "mme_load_clip_text_as", "mme_text_info", "mme_text_forward", "mme_text_apply"):
        assert name in EXPORTS
    for attr in ("load_clip_text", "load_clip_text_checkpoint", "text_info", "text_forward", "text_apply"):
        assert callable(getattr(Engine, attr))
    assert isinstance(Engine.text_embed_dim, property) and Engine.TEXT_OPS == {"token_rows": 0, "attention_causal": 1, "eos_pool_ln": 2}
    assert "clip_text" in ckpt.ENCODERS
    src = os.path.join(HERE, "..", "multimodal_embeddings_amd")
    from multimodal_embeddings_amd import build

    assert {"text_tower.hip", "attention_short.hip", "capi_text.hip"} <= set(build.SOURCES)
    assert all(os.path.exists(os.path.join(src, "csrc", f)) for f in build.SOURCES)


# ---- the attention cases of the GPU test can catch a wrong kernel: float64 only ---------------------------------------
def attention_mutants(qkv, n, heads):
    """name -> (output of a wrong kernel in float64, the rows of every sequence on which it must leave the tolerance)"""
    T = tr.T
    tril = np.tril(np.ones((T, T), dtype=bool))
    strict = np.tril(np.ones((T, T), dtype=bool), -1)
    strict[0, 0] = True  # a strict mask leaves query 0 without a key; any kernel would still have to return something
    shifted = np.tril(np.ones((T, T), dtype=bool), 1)
    padded = np.concatenate([tril, np.ones((T, 96 - T), dtype=bool)], axis=1)  # keys 77..95 admitted: clamped copies of row 76
    return {
        "no mask": (tr.causal_attention_f64(qkv, n, heads, allowed=np.ones((T, T), dtype=bool))[0], range(0, 70)),
        "strict mask (j < i)": (tr.causal_attention_f64(qkv, n, heads, allowed=strict)[0], range(1, 40)),
        "mask shifted by one (j <= i + 1)": (tr.causal_attention_f64(qkv, n, heads, allowed=shifted)[0], range(0, 40)),
        "keys 77..95 admitted": (tr.causal_attention_f64(qkv, n, heads, allowed=padded, keys=96)[0], range(0, T)),
        "missing scale": (tr.causal_attention_f64(qkv, n, heads, q_factor=1.0 / tr.SC)[0], range(8, T)),
    }


def assert_mutants_leave_the_tolerance(qkv, n, heads, ref, A):
    tol = tr.attention_tolerance(ref, A).reshape(n, tr.T, -1)
    for name, (out, rows) in attention_mutants(qkv, n, heads).items():
        far = np.abs(out - ref).reshape(n, tr.T, -1) > 4 * tol
        per_row = far.any(axis=2)[:, list(rows)]
        print(f"mutant '{name}': {int(far.sum())} of {far.size} elements beyond 4 x the tolerance; rows caught {int(per_row.sum())} of {per_row.size}")
        assert per_row.all(), f"mutant '{name}' stays inside 4 x the tolerance on row(s) {np.argwhere(~per_row)[:4].tolist()} of {list(rows)[:3]}.."


@pytest.mark.parametrize("heads", [8, 16])
def test_planted_attention_cases_separate_the_mutants(heads):
    n = 2
    qkv = tr.planted_qkv(n, heads, seed=5)
    ref, A = tr.causal_attention_f64(qkv, n, heads)
    assert np.isfinite(ref).all() and np.array_equal(ref.reshape(n, tr.T, -1)[:, 0], qkv.reshape(n, tr.T, 3, -1)[:, 0, 2].astype(np.float64))
    assert_mutants_leave_the_tolerance(qkv, n, heads, ref, A)
