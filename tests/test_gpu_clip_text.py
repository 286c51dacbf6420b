"""The CLIP text tower on the GPU (csrc/text_tower.hip, attention_short.hip, capi_text.hip): every new kernel one launch at a
time against numpy / float64, the prepared buffers, parity with what transformers returned (tests/golden/clip_text_cases.npz),
bit identities, coexistence with the image tower, the public interface and the refusals.

Tolerances, none fitted:
(1) token rows: bit-equal to numpy's bf16(f32 + f32) -- one add, one rounding to nearest even.
(2) causal attention: |got - ref| <= 2^-8 |ref| + 2^-8 A, A = sum p |v| / sum p from the same float64 pass: the bound
    tests/test_gpu_attention.py derives for a kernel that rounds P to bf16 before P . V and the output to bf16, which are this
    kernel's two rounding points as well.  tests/test_clip_text_cpu.py shows in float64 that the planted cases tell a missing,
    strict or shifted mask, admitted padding and a missing scale from the contract by 4 x that bound.
(3) EOS pool-LN: the yardstick rule of tests/test_gpu_clip.py's pool_ln_rows test: 8 x the deviation of a float32 numpy
    restatement, never below 2^-22 of the largest value, plus the bf16 format's own ulp / 2.
(4) prepared buffers: the definitions and bounds of tests/test_gpu_weight_prep.py.
(5) parity: max(1 - cos) <= 1e-3 against the recorded transformers rows, the project's bound for the CLIP image tower.
    Measured on one MI355X: B 4.4e-5, L2 2.0e-5, H2 2.0e-5, B2n 1.4e-5, V1 1.3e-5.
    What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
    tests/test_gpu_tower_sharpness.py.
A GPU fault in one test ends the module's GPU work: the tests after it fail without launching anything.
"""
import ctypes as C
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
from test_clip_text_cpu import assert_mutants_leave_the_tolerance, toy_tokenizer_files  # noqa: E402
from test_gpu_gemm import BF16, DEV, F32, Guard, assert_bits, assert_close, assert_mutant_far, ulp_bf16  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, VIT_B16, CLIPTextGeometry, bf16_bits_to_f32, f32_to_bf16_bits, make_clip_text_weights,  # noqa: E402
                                               make_clip_weights, make_vit_weights, round_to_bf16, synthetic_crops, synthetic_token_ids)

pytestmark = pytest.mark.gpu

I16 = torch.int16
TT = 77
CHUNK = 1024  # MME_TEXT_CHUNK
T2 = CLIPTextGeometry(num_layers=2, vocab_size=256, eos_token_id=255)  # CLIP-B's text width, two layers: the quick tower
_fault = []


@pytest.fixture(autouse=True)
def _a_fault_ends_the_module():
    if _fault:
        pytest.fail(f"not run: an earlier test of this module met a GPU fault ({_fault[0]})")
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _fault.append(str(e)[:200])
        raise


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "clip_text_cases.npz"))


_weights = {}


def weights_of(key):
    if key not in _weights:
        _weights[key] = make_clip_text_weights(41, T2) if key == "T2" else make_clip_text_weights(mk.CASES[key][0], mk.CASES[key][1])
    return _weights[key]


def bf16_dev(x32: np.ndarray):
    """bf16-representable f32 array -> bf16 CUDA tensor"""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV).to(BF16)


# ---------------------------------------------------------------------------------------------------------------------
# (1) token rows


@pytest.mark.parametrize("d, vocab, special", [(512, 300, (0, 299)), (768, 300, (0, 299)), (1024, 300, (0, 299)), (1024, 49408, (0, 49407))])
def test_token_rows(eng, d, vocab, special):
    n = 3
    rng = np.random.default_rng(d + vocab)
    tok = round_to_bf16(rng.standard_normal((vocab, d)).astype(np.float32))
    pos = (rng.standard_normal((TT, d)) * 0.7).astype(np.float32)  # f32, not bf16-representable: the sum must round once
    ids = rng.integers(0, vocab, size=(n, TT)).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[2, 76], ids[1, 40] = special[0], special[1], special[1], special[0]
    x = Guard(BF16, n * TT, d)
    eng.text_apply("token_rows", tok=bf16_dev(tok), pos=torch.from_numpy(pos).to(DEV), ids=ids, x=x.view, n=n, d=d, vocab=vocab)
    x.check("token_rows")  # the sentinel rows behind n * 77 (and before row 0) are untouched
    want = f32_to_bf16_bits(tok[ids.reshape(-1)] + pos[np.arange(n * TT) % TT]).astype(np.int16)
    assert_bits(x.valid_bits(), torch.from_numpy(want).to(DEV), f"token_rows d {d} vocab {vocab}")
    # sharpness: the position table shifted by one row, and the table row of the neighbouring id
    assert int((f32_to_bf16_bits(tok[ids.reshape(-1)] + pos[(np.arange(n * TT) + 1) % TT]).astype(np.int16) != want).sum()) > n * TT * d // 2
    assert int((f32_to_bf16_bits(tok[(ids.reshape(-1) + 1) % vocab] + pos[np.arange(n * TT) % TT]).astype(np.int16) != want).sum()) > n * TT * d // 2


# ---------------------------------------------------------------------------------------------------------------------
# (2) causal attention


def run_attention(eng, qkv32: np.ndarray, n, heads):
    out = Guard(BF16, n * TT, 64 * heads)
    eng.text_apply("attention_causal", qkv=bf16_dev(qkv32), out=out.view, n=n, heads=heads)
    out.check(f"attention_causal n {n} heads {heads}")  # sentinel rows behind n * 77 untouched
    return out


def check_attention(out, qkv32, n, heads, what):
    ref, A = tr.causal_attention_f64(qkv32, n, heads)
    got = out.valid.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite outputs"
    assert_close(got, torch.from_numpy(ref).to(DEV), torch.from_numpy(tr.attention_tolerance(ref, A)).to(DEV), what)
    # row 0 of every (sequence, head) is a softmax over one key: V[0], bit for bit
    v0 = bf16_dev(qkv32.reshape(n, TT, 3, 64 * heads)[:, 0, 2])
    assert_bits(out.valid.view(n, TT, 64 * heads)[:, 0].contiguous().view(I16), v0.view(I16), f"{what}: row 0 == V[0]")
    return ref, A


@pytest.mark.parametrize("n, heads", [(n, h) for h in (8, 12, 16) for n in (1, 2, 3, 5, 64)] + [(257, 8)])
def test_attention_causal_against_float64(eng, n, heads):
    qkv = tr.planted_qkv(n, heads, seed=100 + n)
    check_attention(run_attention(eng, qkv, n, heads), qkv, n, heads, f"attention_causal n {n} heads {heads}")


@pytest.mark.parametrize("heads", [8, 16])
def test_attention_causal_planted_cases(eng, heads):
    n = 2
    qkv = tr.planted_qkv(n, heads, seed=5)  # the inputs of tests/test_clip_text_cpu.py::test_planted_attention_cases_separate_the_mutants
    ref, A = check_attention(run_attention(eng, qkv, n, heads), qkv, n, heads, f"planted attention heads {heads}")
    assert_mutants_leave_the_tolerance(qkv, n, heads, ref, A)


@pytest.mark.parametrize("heads", [8, 12])
def test_attention_causal_ignores_the_future_bit_for_bit(eng, heads):
    n, D = 3, 64 * heads
    a = tr.planted_qkv(n, heads, seed=9)
    b = a.copy().reshape(n, TT, 3, D)
    rng = np.random.default_rng(3)
    big = round_to_bf16((rng.choice([-1.0, 1.0], size=(n, TT - 41, 2, D)) * rng.choice([1e3, 1e18, 1e30, 3e38], size=(n, TT - 41, 2, D))).astype(np.float32))
    assert np.isfinite(big).all()
    b[:, 41:, 1:] = big  # K and V rows j > 40 of every sequence: large finite values
    b = b.reshape(n * TT, 3 * D)
    oa, ob = run_attention(eng, a, n, heads), run_attention(eng, b, n, heads)
    ga, gb = oa.valid.view(n, TT, D)[:, :41].contiguous(), ob.valid.view(n, TT, D)[:, :41].contiguous()
    assert bool(torch.isfinite(gb.float()).all())
    assert_bits(gb.view(I16).view(n * 41, D), ga.view(I16).view(n * 41, D), "rows 0..40 with other K / V rows behind them")


# ---------------------------------------------------------------------------------------------------------------------
# (3) EOS pool-LN


def ln_ref_np(x, gamma, beta, eps, dtype):
    x, gamma, beta = x.astype(dtype), gamma.astype(dtype), beta.astype(dtype)
    mean = x.mean(1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(eps)) * gamma + beta


@pytest.mark.parametrize("d", [512, 768, 1024])
def test_eos_pool_ln(eng, d):
    eps = 1e-5
    pos = np.array([0, 1, 31, 32, 76], dtype=np.int32)  # mixed in one batch
    B = len(pos)
    rng = np.random.default_rng(700 + d)
    xh = rng.standard_normal((B * TT, d)).astype(np.float32)
    xh[1 * TT + 1] += 30.0
    xh[2 * TT + 31] *= 100.0
    xh[3 * TT + 32] = 0.0  # a zero row: beta
    gamma = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
    X = torch.from_numpy(xh).to(DEV).to(BF16)
    y, yf = Guard(BF16, B, d), Guard(F32, B, d)
    eng.text_apply("eos_pool_ln", x=X, gamma=torch.from_numpy(gamma).to(DEV), beta=torch.from_numpy(beta).to(DEV), eos_pos=pos, y=y.view, y_f32=yf.view,
                   n=B, d=d, eps=eps)
    y.check("eos_pool_ln bf16")
    yf.check("eos_pool_ln f32")
    rows = X.view(B, TT, d)[torch.arange(B), torch.from_numpy(pos).long()].float().cpu().numpy()
    e32 = float(np.float32(eps))
    ref = ln_ref_np(rows, gamma, beta, e32, np.float64)
    yard = float(np.abs(ln_ref_np(rows, gamma, beta, e32, np.float32).astype(np.float64) - ref).max())
    floor = max(8 * yard, 2.0**-22 * float(np.abs(ref).max()))
    reft = torch.from_numpy(ref).to(DEV)
    tol = ulp_bf16(reft) / 2 + floor
    print(f"eos_pool_ln d {d}: float32 yardstick {yard:.3g}")
    assert_close(y.valid.double(), reft, tol, f"eos_pool_ln d {d} bf16")
    assert_close(yf.valid.double(), reft, torch.full_like(reft, floor), f"eos_pool_ln d {d} f32")
    assert_bits(y.valid_bits(), yf.valid.to(BF16).view(I16), "the bf16 rows are the f32 rows rounded once")
    assert_bits(y.valid[3].view(I16)[None], torch.from_numpy(beta).to(DEV).to(BF16).view(I16)[None], "zero row: beta")
    other = X.view(B, TT, d)[torch.arange(B), torch.from_numpy((pos + 1) % TT).long()].float().cpu().numpy()
    assert_mutant_far(torch.from_numpy(ln_ref_np(other, gamma, beta, e32, np.float64)).to(DEV), reft, tol, B * d // 2, "the row behind the EOS pooled")
    same = X.view(B, TT, d)[:, 0].float().cpu().numpy()
    assert_mutant_far(torch.from_numpy(ln_ref_np(same, gamma, beta, e32, np.float64)).to(DEV)[1:], reft[1:], tol[1:], (B - 1) * d // 2, "one position for every sequence")


# ---------------------------------------------------------------------------------------------------------------------
# (4) prepared buffers


def text_table(m, g):
    import test_gpu_weight_prep as wp

    t_ = "text_model."
    s = 64 ** -0.5 * wp.LOG2E
    t = [("tok", "bf16", m[t_ + "embeddings.token_embedding.weight"]), ("pos", "f32", m[t_ + "embeddings.position_embedding.weight"]),
         ("lnf_g", "f32", m[t_ + "final_layer_norm.weight"]), ("lnf_b", "f32", m[t_ + "final_layer_norm.bias"])]
    for l in range(g.num_layers):
        p = f"{t_}encoder.layers.{l}."
        qkv = dict(W=[m[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], b=[m[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], s=[s, None, None],
                   gamma=m[p + "layer_norm1.weight"], beta=m[p + "layer_norm1.bias"], eps=g.layer_norm_eps)
        fc1 = dict(W=[m[p + "mlp.fc1.weight"]], b=[m[p + "mlp.fc1.bias"]], s=[None], gamma=m[p + "layer_norm2.weight"], beta=m[p + "layer_norm2.bias"],
                   eps=g.layer_norm_eps)
        t += [(f"{l}.qkv_wf", "fold", qkv), (f"{l}.qkv_cs", "cs", qkv), (f"{l}.qkv_bf", "bf", qkv),
              (f"{l}.o_w", "bf16", m[p + "self_attn.out_proj.weight"]), (f"{l}.o_b", "f32", m[p + "self_attn.out_proj.bias"]),
              (f"{l}.fc1_wf", "fold", fc1), (f"{l}.fc1_cs", "cs", fc1), (f"{l}.fc1_bf", "bf", fc1),
              (f"{l}.fc2_w", "bf16", m[p + "mlp.fc2.weight"]), (f"{l}.fc2_b", "f32", m[p + "mlp.fc2.bias"])]
    if g.projection_dim:
        t.append(("proj_w", "bf16", m["text_projection.weight"]))
    return t


@pytest.mark.parametrize("case", [("bfloat16", CLIPTextGeometry(num_layers=2, intermediate_size=128, vocab_size=96, eos_token_id=95, projection_dim=192, hidden_act="gelu")),
                                  ("float16", CLIPTextGeometry(hidden_size=1024, num_layers=1, num_heads=16, intermediate_size=64, vocab_size=40, eos_token_id=2,
                                                               projection_dim=None)),
                                  ("float32", CLIPTextGeometry(hidden_size=768, num_layers=1, num_heads=12, intermediate_size=64, vocab_size=40, eos_token_id=39,
                                                               projection_dim=64))],
                         ids=["512x2-bf16", "1024x1-f16-noproj", "768x1-f32"])
def test_prepared_buffers(tmp_path, case):
    import test_gpu_weight_prep as wp

    dtype, geom = case
    ckpt.save_checkpoint(tmp_path, make_clip_text_weights(21, geom), "clip_text", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "clip_text")
    assert ck.dtype == dtype and ck.geometry == geom
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_clip_text_checkpoint(ck)
        host.load_clip_text({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (bd, fd), (bh, fh) = wp._read_all(dev), wp._read_all(host)
        info = dev.text_info()
        assert dev.text_embed_dim == geom.embed_dim and dev.encoder_info()["kind"] == "vit"  # the image side is untouched
    finally:
        dev.close()
        host.close()
    L = geom.num_layers
    assert info == {"loaded": 1, "hidden_size": geom.hidden_size, "num_layers": L, "num_heads": geom.num_heads, "intermediate_size": geom.intermediate_size,
                    "vocab_size": geom.vocab_size, "projection_dim": geom.projection_dim, "hidden_act": geom.hidden_act, "eos_token_id": geom.eos_token_id}
    assert len(bd) == len(bh) == 4 + 10 * L + (1 if geom.projection_dim else 0) and fd == fh  # host- and device-prepared fingerprints are equal
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    wp.DEV_OF[0] = DEV
    m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    folds = wp.check_table(text_table(m, geom), bd, f"clip_text {dtype}")
    assert len(folds) == 2 * L
    for k, (name, (d, out)) in enumerate(folds.items()):  # the folds sit under layer_norm1 / layer_norm2
        left, right, tol, (x, xc, r, W, b) = wp.function_check(name, d, out, 300 + k, f"clip_text {dtype}")
        other = [dd for nme, (dd, _) in folds.items() if nme[:2] == name[:2] and nme != name]
        gm, bt = other[0]["gamma"].double(), other[0]["beta"].double()
        assert_mutant_far((gm * xc * r + bt) @ W.T + b[None], right, tol, right.numel() // 2, f"{name}: the other LayerNorm's gamma and beta")


# ---------------------------------------------------------------------------------------------------------------------
# (5) parity with transformers


@pytest.mark.parametrize("key", list(mk.CASES))
def test_parity_with_the_recorded_transformers_rows(recorded, key):
    seed, geom, _, _ = mk.CASES[key]
    ids = recorded[f"{key}.ids"]
    rec = recorded[f"{key}.text_embeds" if geom.projection_dim else f"{key}.pooler_output"]
    e = Engine(0)
    try:
        e.load_clip_text(weights_of(key), geom)
        assert e.text_embed_dim == geom.embed_dim
        e32, e16 = e.text_forward(ids)
        torch.cuda.synchronize()
    finally:
        e.close()
    got = e32.cpu().numpy()
    assert got.shape == (mk.N_SEQ, geom.embed_dim) and np.isfinite(got).all()
    assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
    omc = tr.one_minus_cos(got, rec)
    print(f"text parity {key}: max(1 - cos) against transformers = {omc.max():.3g} (bound 1e-3), per sequence length {dict(zip(mk.LENGTHS, np.round(omc, 7)))}")
    assert float(omc.max()) <= 1e-3
    # sharpness: the row before the EOS of the same sequences is far outside the bound
    ref = tr.clip_text_embed(ids, weights_of(key), geom)
    assert float(tr.one_minus_cos(got, ref).max()) <= 1e-3
    early = ids.copy()
    for i, n in enumerate(mk.LENGTHS[2:], start=2):
        early[i, n - 2 :] = mk.CASES[key][2]
    wrong = tr.one_minus_cos(tr.clip_text_embed(early[2:], weights_of(key), geom), rec[2:])
    print(f"text parity {key}: the row before the EOS pooled instead: min(1 - cos) = {wrong.min():.3g}")
    assert float(wrong.min()) > 4e-3


# ---------------------------------------------------------------------------------------------------------------------
# (6) identities


@pytest.fixture(scope="module")
def t2eng():
    e = Engine(0)
    e.load_clip_text(weights_of("T2"), T2)
    yield e
    e.close()


def test_permutation_padding_and_output_forms(t2eng):
    e = t2eng
    lengths = [2, 3, 16, 31, 32, 33, 64, 65, 76, 77, 40, 50]
    ids = synthetic_token_ids(len(lengths), T2.vocab_size, T2.eos_token_id, 11, lengths)
    e32, e16 = e.text_forward(ids)
    perm = np.random.default_rng(0).permutation(len(lengths))
    p32, _ = e.text_forward(ids[perm])
    assert torch.equal(p32.view(torch.int32), e32[torch.from_numpy(perm).to(DEV)].view(torch.int32))  # a permuted batch permutes the rows
    zero = ids.copy()
    for i, n in enumerate(lengths):
        zero[i, n:] = 0  # padding with id 0 instead of the eos id: the first-occurrence rule pools the same row
    z32, _ = e.text_forward(zero)
    assert torch.equal(z32.view(torch.int32), e32.view(torch.int32))
    assert torch.equal(e16.view(I16), e32.to(BF16).view(I16))  # f32 and bf16 outputs are consistent
    only16 = e.text_forward(ids, want_f32=False)
    assert only16[0] is None and torch.equal(only16[1].view(I16), e16.view(I16))
    assert np.allclose(np.linalg.norm(e32.double().cpu().numpy(), axis=1), 1.0, atol=1e-6)
    z = e.text_forward(np.zeros((0, TT), dtype=np.int32))
    assert tuple(z[0].shape) == (0, T2.embed_dim) and tuple(z[1].shape) == (0, T2.embed_dim)  # n = 0 gives empty
    ref = tr.clip_text_embed(ids, weights_of("T2"), T2)
    assert float(tr.one_minus_cos(e32.cpu().numpy(), ref).max()) <= 1e-3


def test_a_batch_larger_than_the_chunk_equals_two_calls(t2eng):
    e = t2eng
    n = CHUNK + 3
    ids = synthetic_token_ids(n, T2.vocab_size, T2.eos_token_id, 12)
    whole, _ = e.text_forward(ids, want_bf16=False)
    a, _ = e.text_forward(ids[:CHUNK], want_bf16=False)
    b, _ = e.text_forward(ids[CHUNK:], want_bf16=False)
    assert torch.equal(whole.view(torch.int32), torch.cat([a, b]).view(torch.int32))
    assert bool(torch.isfinite(whole).all())


# ---------------------------------------------------------------------------------------------------------------------
# (7) coexistence


def _image_rows(e, crops):
    hw = np.tile(np.array([[224, 224]], dtype=np.int32), (crops.shape[0], 1))
    offs = np.arange(crops.shape[0], dtype=np.int64) * (224 * 224 * 3)
    return e.embed(crops.reshape(-1), offs, hw, want_bf16=False)[0]


def test_text_and_image_towers_share_a_context():
    crops = torch.from_numpy(synthetic_crops(40, seed=3)).to(DEV)
    ids = synthetic_token_ids(6, T2.vocab_size, T2.eos_token_id, 13, [2, 20, 33, 64, 70, 77])
    g_img = dataclasses.replace(CLIP_B16, num_layers=2)
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip(make_clip_weights(15, g_img), g_img)
        before = _image_rows(e, crops).clone()
        n_img = len(e.weights_fingerprint())
        e.load_clip_text(weights_of("T2"), T2)
        fp = e.weights_fingerprint()
        n_text = 4 + 10 * T2.num_layers + 1
        assert len(fp) == n_img + n_text
        assert torch.equal(_image_rows(e, crops).view(torch.int32), before.view(torch.int32))  # the text load does not touch the image tower
        t0 = e.text_forward(ids, want_bf16=False)[0].clone()
        text_fp = fp[n_img:]
        # image reloads afterwards: they free only their own buffers, the text buffers move down in the table and stay
        e.load_vit(make_vit_weights(1, dataclasses.replace(VIT_B16, num_layers=1)), geom=dataclasses.replace(VIT_B16, num_layers=1))
        assert e.text_info()["loaded"] == 1 and e.encoder_info()["kind"] == "vit"
        fp = e.weights_fingerprint()
        assert fp[:n_text] == text_fp and len(fp) == n_text + 6 + 18
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(torch.int32), t0.view(torch.int32))
        e.load_clip(make_clip_weights(15, g_img), g_img)
        fp = e.weights_fingerprint()
        assert fp[:n_text] == text_fp and len(fp) == n_text + n_img
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(torch.int32), t0.view(torch.int32))
        assert torch.equal(_image_rows(e, crops).view(torch.int32), before.view(torch.int32))
        # a second text load with other weights frees exactly the first
        e.load_clip_text(make_clip_text_weights(42, T2), T2)
        fp2 = e.weights_fingerprint()
        assert len(fp2) == n_text + n_img and fp2[:n_img] == fp[n_text:] and fp2[n_img:] != text_fp
        t1 = e.text_forward(ids, want_bf16=False)[0]
        assert float((t1 - t0).abs().max()) > 1e-2
        assert torch.equal(_image_rows(e, crops).view(torch.int32), before.view(torch.int32))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (8) the public interface


def _close_all(emb):
    for e in emb.engines:
        e.close()


def test_region_embedder_seeded_text_tower():
    emb = RegionEmbedder(device=0, encoder="clip", text_tower=True, chunk=64)  # seeded on both sides
    try:
        info = emb.engine.text_info()
        assert info["loaded"] == 1 and (info["hidden_size"], info["num_layers"], info["vocab_size"], info["eos_token_id"]) == (512, 12, 49408, 49407)
        assert emb.text_embed_dim == emb.embed_dim == 512
        v = emb.get_text_embeddings([5, 6, 7, 49407])
        assert isinstance(v, list) and len(v) == emb.embed_dim and abs(float(np.linalg.norm(np.array(v, dtype=np.float64))) - 1.0) <= 1e-6
        assert emb.get_text_embeddings([5, 6, 7]) == v  # right-padded with the eos id: the same sequence
        both = emb.get_text_embeddings(np.array([[5, 6, 7, 49407], [9, 49407, 0, 0]]))
        assert len(both) == 2 and both[0] == v and both[1] != v
        with pytest.raises(MmeError, match="sequence 0 holds no eos_token_id = 49407"):
            emb.get_text_embeddings(list(range(77)))
        with pytest.raises(MmeError, match="token ids .* are accepted"):
            emb.get_text_embeddings("a seeded tower brings no tokenizer")
        assert emb.get_text_embeddings([5, 6, 7, 49407]) == v  # still usable
    finally:
        _close_all(emb)


def test_text_queries_through_the_toy_tokenizer(tmp_path):
    from transformers import CLIPTokenizer

    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    toy_tokenizer_files(tmp_path / "tok")
    g_img = dataclasses.replace(CLIP_B16, num_layers=2)
    g_txt = dataclasses.replace(T2, vocab_size=195, eos_token_id=194)  # the toy vocabulary: <|endoftext|> = 194, the last id
    emb = RegionEmbedder(device=0, encoder="clip", weights=make_clip_weights(15, g_img), geometry=g_img, chunk=64,
                         text_tower=make_clip_text_weights(44, g_txt), tokenizer=CLIPTokenizer.from_pretrained(str(tmp_path / "tok"), local_files_only=True))
    try:
        assert emb.engine.text_info()["eos_token_id"] == 194 and emb.text_embed_dim == emb.embed_dim == 512
        s = emb.get_text_embeddings("The news")  # the string path
        assert len(s) == 512 and s == emb.get_text_embeddings([193, 189, 192, 194])
        both = emb.get_text_embeddings(["The news", "news"])  # the list form
        assert len(both) == 2 and both[0] == s and both[1] != s
        # image vectors in a collection, queried by text and by the same vectors
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(24, seed=8)), as_array=True)
        assert ok.all()
        col = RegionCollection()
        col.upsert(ids=[f"region_{r}" for r in range(24)], embeddings=rows.tolist(),
                   metadatas=[{"parent_image": f"/p/{r // 4}.png", "region_type": "plain_text", "box_str": "0,0,1,1", "area_percentage": 1.0, "is_region": True}
                              for r in range(24)])
        texts = ["The news", "news"]
        by_text = col.query(query_texts=texts, embedder=emb, n_results=5, engine=emb.engine)
        by_vec = col.query(query_embeddings=[emb.get_text_embeddings(t) for t in texts], n_results=5, engine=emb.engine)
        assert by_text == by_vec and len(by_text["ids"]) == 2 and len(by_text["ids"][0]) == 5
        one = col.query(query_texts="The news", embedder=emb, n_results=5, engine=emb.engine)
        assert one["ids"] == by_text["ids"][:1] and one["distances"] == by_text["distances"][:1]
        narrow = RegionCollection()
        narrow.upsert(ids=["a", "b"], embeddings=np.eye(2, 64).tolist(), metadatas=[{"parent_image": "/p/0.png"}] * 2)
        with pytest.raises(ValueError, match="512 dimensions, the stored vectors have 64"):
            narrow.query(query_texts=texts, embedder=emb, engine=emb.engine)
    finally:
        _close_all(emb)


def test_region_embedder_without_a_tower_stays_a_stub():
    emb = RegionEmbedder(device=0, encoder="clip", chunk=64)  # seeded, text_tower=None: nothing to load lazily
    try:
        assert emb.engine.text_info()["loaded"] == 0 and emb.text_embed_dim == 0
        with pytest.raises(NotImplementedError):
            emb.get_text_embeddings([1, 2, 49407])
    finally:
        _close_all(emb)
    off = RegionEmbedder(device=0, encoder="clip", chunk=64, text_tower=False)
    try:
        with pytest.raises(NotImplementedError):
            off.get_text_embeddings("x")
    finally:
        _close_all(off)


def test_lazy_load_from_a_whole_clip_model_directory(tmp_path):
    from safetensors.torch import save_file

    g_img = dataclasses.replace(CLIP_B16, num_layers=1, intermediate_size=256, projection_dim=128)
    g_txt = dataclasses.replace(T2, intermediate_size=256, projection_dim=128, vocab_size=195, eos_token_id=194)  # the toy vocabulary
    tw = make_clip_text_weights(43, g_txt)
    whole = dict(make_clip_weights(16, g_img))
    whole.update(tw)
    whole["logit_scale"] = np.float32([2.6592])
    d = tmp_path / "clip"
    os.makedirs(d)
    cfg = {"model_type": "clip", "projection_dim": 128,
           "text_config": {"vocab_size": g_txt.vocab_size, "hidden_size": 512, "num_hidden_layers": 2, "num_attention_heads": 8, "intermediate_size": 256,
                           "max_position_embeddings": 77, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5, "eos_token_id": g_txt.eos_token_id},
           "vision_config": {"image_size": 224, "patch_size": 16, "hidden_size": 768, "num_hidden_layers": 1, "num_attention_heads": 12,
                             "intermediate_size": 256, "hidden_act": "quick_gelu", "layer_norm_eps": 1e-5}}
    json.dump(cfg, open(d / "config.json", "w"))
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).contiguous() for k, v in whole.items()}, str(d / "model.safetensors"),
              metadata={"format": "pt"})
    toy_tokenizer_files(d)  # vocab.json / merges.txt beside the weights: the lazy CLIPTokenizer finds them
    emb = RegionEmbedder(str(d), device=0, encoder="clip", chunk=64)
    try:
        assert emb.embed_dim == 128 and emb.engine.text_info()["loaded"] == 0  # nothing text-side exists before the first call
        n_img = len(emb.engine.weights_fingerprint())
        v = emb.get_text_embeddings("The news")
        assert emb.engine.text_info()["loaded"] == 1 and len(v) == 128 and len(emb.engine.weights_fingerprint()) == n_img + 4 + 20 + 1
        row = np.full((1, TT), 194, dtype=np.int64)
        row[0, :3] = [193, 189, 192]  # what the tokenizer makes of "The news"
        assert v == emb.get_text_embeddings(row[0])
        want = tr.clip_text_embed(row, tw, g_txt)  # the bf16 file holds the seeded values exactly
        assert float(tr.one_minus_cos(np.array(v, dtype=np.float64)[None], want).max()) <= 1e-3
        rows, ok = emb.get_image_embeddings(list(synthetic_crops(2, seed=8)), as_array=True)  # the image side still runs
        assert ok.all() and rows.shape == (2, 128)
    finally:
        _close_all(emb)


# ---------------------------------------------------------------------------------------------------------------------
# (9) refusals through the C ABI


def test_refusals_leave_the_context_usable():
    e = Engine(0)
    try:
        ids = synthetic_token_ids(3, T2.vocab_size, T2.eos_token_id, 14, [2, 40, 77])
        with pytest.raises(MmeError, match="call mme_load_clip_text first"):
            e.text_forward(ids)  # forward before load
        bad = dataclasses.replace(T2, hidden_size=640, num_heads=10)
        w640 = make_clip_text_weights(1, dataclasses.replace(bad, num_layers=1, intermediate_size=64, vocab_size=8, eos_token_id=7))
        with pytest.raises(MmeError, match=r"hidden = 640; supported: 512, 768, 1024"):
            e.load_clip_text(w640, dataclasses.replace(bad, num_layers=1, intermediate_size=64, vocab_size=8, eos_token_id=7))
        assert e.text_info()["loaded"] == 0 and len(e.weights_fingerprint()) == 0
        e.load_clip_text(weights_of("T2"), T2)
        good = e.text_forward(ids, want_bf16=False)[0].clone()
        fp = e.weights_fingerprint()
        for change, text in ((dict(num_heads=12), "heads = 12 at hidden = 512"), (dict(max_position_embeddings=64), "max_positions = 64; supported: 77"),
                             (dict(projection_dim=96), "proj_dim = 96"), (dict(eos_token_id=T2.vocab_size), "eos_token_id = 256")):
            g = dataclasses.replace(T2, **change)
            W, layers = Engine._weights_struct("clip_text", g, lambda name: None)  # geometry only: refused before any tensor is read
            assert e.lib.mme_load_clip_text(e.h, C.byref(W)) != 0 and text in e.lib.mme_last_error(e.h).decode(), change
            assert e.weights_fingerprint() == fp and e.text_info()["loaded"] == 1  # a refusal leaves the context unchanged
        # ids: straight at the C ABI, then through Engine.text_forward (which adds no check of its own)
        out = torch.empty((3, T2.embed_dim), dtype=F32, device=DEV)

        def raw(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            rc = e.lib.mme_text_forward(e.h, a.ctypes.data, a.shape[0], out.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            return rc, e.lib.mme_last_error(e.h).decode()

        oob = ids.copy()
        oob[1, 7] = T2.vocab_size
        rc, msg = raw(oob)
        assert rc != 0 and "sequence 1, position 7: id = 256" in msg
        neg = ids.copy()
        neg[2, 0] = -1
        assert raw(neg)[0] != 0
        no_eos = ids.copy()
        no_eos[2] = 9
        rc, msg = raw(no_eos)
        assert rc != 0 and "sequence 2 holds no eos_token_id = 255" in msg
        with pytest.raises(MmeError, match="sequence 2 holds no eos_token_id = 255"):
            e.text_forward(no_eos)
        with pytest.raises(MmeError, match="sequence 1, position 7"):
            e.text_forward(oob)
        with pytest.raises(MmeError, match=r"\[n, 77\]"):
            e.text_forward(ids[:, :76])
        rc, _ = raw(ids)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out.view(torch.int32), good.view(torch.int32))  # the next valid call succeeds, same bits
        # the one-launch diagnostic refuses what it cannot run
        x = torch.zeros((TT, 512), dtype=BF16, device=DEV)
        f = torch.zeros((TT * 512,), dtype=F32, device=DEV)
        with pytest.raises(MmeError, match="d == 512, d == 768 and d == 1024"):
            e.text_apply("token_rows", tok=x, pos=f, ids=np.zeros((1, TT)), x=x, n=1, d=384, vocab=TT)
        with pytest.raises(MmeError, match=r"ids_host\[3\] = 77 outside"):
            e.text_apply("token_rows", tok=x, pos=f, ids=np.array([[0, 1, 2, 77] + [0] * 73]), x=x, n=1, d=512, vocab=TT)
        with pytest.raises(MmeError, match="heads == 8, 12 and 16"):
            e.text_apply("attention_causal", qkv=x, out=x, n=1, heads=6)
        with pytest.raises(MmeError, match=r"eos_pos_host\[0\] = 77 outside 0..76"):
            e.text_apply("eos_pool_ln", x=x, gamma=f, beta=f, eos_pos=[77], y=x, n=1, d=512)
        with pytest.raises(MmeError, match="op 7 outside 0..2"):
            e.text_apply(7, n=1)
        assert torch.equal(e.text_forward(ids, want_bf16=False)[0].view(torch.int32), good.view(torch.int32))
    finally:
        e.close()
