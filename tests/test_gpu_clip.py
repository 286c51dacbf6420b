"""CLIP ViT/16 image towers on the GPU: the kernels the tower adds, one launch at a time (mme_clip_apply) against float64;
the prepared weight buffers; the whole pass against the float32 restatement of tests/clip_reference.py and against the rows
transformers itself returned (tests/golden/clip_cases.npz); bit identities; reloads; downstream kernels at d = 512; refusals.

(1) QuickGELU epilogues (ops 0, 1): x * sigmoid(1.702 x) element by element against float64 on pre-activations known exactly
    (the dense grid of tests/test_gpu_gemm.py: > 10^5 distinct values of [-12, 12], +-0, +-2^-100, +-100, +-3e38).
    Tolerance  ulp_bf16(ref)/2 (1 + 2^-6) + 8 * 2^-24 (1 + |x|) |ref| + 2^-126,  derived, nothing fitted:
    the kernel computes h = v_exp_f32(f32(x C/2)) with C = f32(-1.702 log2 e) (C/2 is the same f32 one exponent lower),
    s = fma(h, h 2^-8, 2^-8) = 2^-8 (1 + e) with e = h^2, r = v_rcp_f32(s), y = f32(f32(x 2^-8) r); the factors 2^-8 are exact and
    keep every intermediate inside the f32 range for as long as the result is a normal number (gemm_epilogue.h).  Relative
    errors, in units of 2^-24 (v_exp_f32 and v_rcp_f32 are 1 ulp = 2 units; a correctly rounded operation is 1 unit):
      - the rounding of C and of the product x C/2: one unit each of the argument t = x C, which changes e = 2^t relatively
        by ln 2 |t| = 1.702 |x| per unit: 3.404 |x|;  v_exp_f32 gives h within 2 units, so e = h^2 within 4;  a relative error
        of e enters sigmoid = 1 / (1 + e) times e / (1 + e) <= 1;
      - the fma 1, v_rcp_f32 2, the last product 1.
    Sum: 2^-24 (8 + 3.404 |x|) |ref| <= 8 * 2^-24 (1 + |x|) |ref|.  2^-126 covers a flushed subnormal (h^2 2^-8 or the result
    below the smallest normal f32 becomes 0); the first term is the final bf16 rounding as in that file.
    On random data the pre-activation itself carries that file's accumulation bound d = K 2^-23 sum|a w| + 4 * 2^-24
    (|acc| + |bias|), which passes through the activation times at most max |d/dx x sigmoid(1.702 x)| < 1.1 (checked here).
(2) pre_ln_rows: the output within the layernorm_rows tolerance of tests/test_gpu_gemm.py (e = d 2^-23), the statistics
    BIT-EQUAL to ln_stats_canonical_rows run on the kernel's own output.
(3) pool_ln_rows, l2_rows: float64 with the yardstick rule of test_pool_ln_l2 there: 8 x the deviation of a float32 numpy
    restatement, measured in the test, never below 2^-22 of the largest value; pool_ln_rows writes bf16, so the format's own
    rounding ulp_bf16(ref)/2 is added.
(5) max(1 - cos) <= 1e-3 against the float32 restatement: the project's bound for the bf16 path against an f32 restatement
    (tests/test_gpu_vit_family.py).  Measured values: DESIGN.md 4.7.
    What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
    tests/test_gpu_tower_sharpness.py.
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

import clip_reference as cr  # noqa: E402
import make_clip_golden as mk  # noqa: E402
from test_gpu_gemm import (BF16, DEV, F32, F64, NP, T, Guard, _gen, _randn, absacc64, acc64, assert_bits, assert_close, assert_mutant_far,  # noqa: E402
                           expect_256, gelu_grid, gelu_ref, ln_rows, stats_ref, ulp_bf16)

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, VIT_B16, CLIPGeometry, make_clip_weights, make_vit_weights, round_to_bf16,  # noqa: E402
                                               synthetic_crops)

pytestmark = pytest.mark.gpu

I16, I32 = torch.int16, torch.int32
CASES = mk.CASES  # B: CLIP-B/16; S2: 384 x 2, gelu, P 256; L3: 1024 x 3, quick_gelu, P 768; B2: CLIP-B width x 2 without projection
B2P = dataclasses.replace(CLIP_B16, num_layers=2)  # CLIP-B width x 2 layers with the 512-d projection: the quick d = 512 tower
_weights = {}


def weights_of(key):
    if key not in _weights:
        _weights[key] = make_clip_weights(15, B2P) if key == "B2P" else make_clip_weights(*CASES[key])
    return _weights[key]


def geom_of(key):
    return B2P if key == "B2P" else CASES[key][1]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (1) QuickGELU


def qgelu_ref(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_tol(ref, x):
    return ulp_bf16(ref) / 2 * (1 + 2.0**-6) + 8 * 2.0**-24 * (1 + x.abs()) * ref.abs() + 2.0**-126


def qlaunch(eng, op, A, W, variant, bias, what):
    M, N = A.shape[0], W.shape[0]
    buf = Guard(BF16, M, N)
    kw = {}
    if op == 1:  # planted statistics (0, 1) and a zero colsum: the folded form reduces to acc + bias exactly
        st = torch.zeros((M, 2), dtype=F32, device=DEV)
        st[:, 1] = 1.0
        kw = dict(ln_stats=st, colsum=torch.zeros(N, dtype=F32, device=DEV))
    ran = eng.clip_apply(op, A=A, W=W, variant=variant, bias=bias, out=buf.view, ldo=buf.ld, **kw)
    want = expect_256(variant, M, N, A.shape[1])  # which kernel a launch must run (tests/test_gpu_gemm.py)
    assert ran == want, f"{what}: ran_256 = {ran}, expected {want}"
    buf.check(what)
    return buf.valid.clone()


@pytest.mark.parametrize("op", [0, 1])
def test_quick_gelu_dense_grid_fast_and_slow_path(eng, op):
    A, W, x = gelu_grid()
    M, N = x.shape
    assert torch.equal(acc64(A, W), x) and torch.equal(x.float().double(), x)
    core = x[x.abs() <= 12]
    assert int(torch.unique(core).numel()) >= 100_000
    for v in (0.0, 2.0**-100, 100.0):
        assert bool((x == v).any()) and bool((x == -v).any()), v
    assert bool((x > 2.9e38).any()) and bool((x < -2.9e38).any())
    bias = torch.zeros(N, dtype=F32, device=DEV)
    ref = qgelu_ref(x)
    tol = qgelu_tol(ref, x)
    outs = {}
    for variant in (1, 3, 4):  # 3, 4: four interior 256 x 256 tiles (fast path); 1: epi_store (slow path)
        w = f"QuickGELU op {op} variant {variant}"
        outs[variant] = qlaunch(eng, op, A, W, variant, bias, w)
        assert_close(outs[variant].double(), ref, tol, w)
    assert torch.equal(outs[1].view(I16), outs[3].view(I16)), "slow-path and fast-path QuickGELU differ in bits"
    assert torch.equal(outs[4].view(I16), outs[3].view(I16))
    out = qlaunch(eng, op, A[:, :64].contiguous(), W[:, :64].contiguous(), 3, bias, "QuickGELU K = 64")  # the 128 x 128 kernel whatever the variant
    assert torch.equal(out.view(I16), outs[1].view(I16))
    fin = x.abs() < 1e30
    assert_mutant_far(gelu_ref(x)[fin], ref[fin], tol[fin], 2000, "erf-GELU")
    assert_mutant_far((x * torch.sigmoid(x))[fin], ref[fin], tol[fin], 2000, "x sigmoid(x)")
    assert_mutant_far(torch.sigmoid(1.702 * x)[fin], ref[fin], tol[fin], 2000, "sigmoid(1.702 x) without the x")


@pytest.mark.parametrize("op", [0, 1])
def test_quick_gelu_takes_the_bias_first(eng, op):
    """x = a_m + bias[n] exactly: a multiples of 2^-4 below 16, bias multiples of 2^-6 in [-2, 2)."""
    M, N, K = 512, 256, 128
    a = ((torch.arange(M, device=DEV, dtype=F64) - 256) / 16).to(BF16)
    bias = ((torch.arange(N, device=DEV, dtype=F64) - 128) / 64).float()
    A = torch.zeros((M, K), dtype=BF16, device=DEV)
    W = torch.zeros((N, K), dtype=BF16, device=DEV)
    A[:, 0] = a
    W[:, 0] = 1.0
    x = a.double()[:, None] + bias.double()[None, :]
    assert torch.equal(x.float().double(), x)
    ref = qgelu_ref(x)
    tol = qgelu_tol(ref, x)
    outs = []
    for variant in (1, 3, 4):
        w = f"QuickGELU + bias op {op} variant {variant}"
        outs.append(qlaunch(eng, op, A, W, variant, bias, w))
        assert_close(outs[-1].double(), ref, tol, w)
    assert torch.equal(outs[0].view(I16), outs[1].view(I16)) and torch.equal(outs[1].view(I16), outs[2].view(I16))
    assert_mutant_far(qgelu_ref(a.double()[:, None] + 0 * x) + bias.double()[None, :], ref, tol, ref.numel() // 2, "bias added after QuickGELU")


@pytest.mark.parametrize("op", [0, 1])
def test_quick_gelu_ragged_shape_random_data(eng, op):
    M, N, K = 394, 384, 128
    g = _gen(90 + op)
    A, W = _randn((M, K), g, 1.0, BF16), _randn((N, K), g, 0.25, BF16)
    bias = _randn((N,), g, 0.5)
    acc = acc64(A, W)
    x = acc + bias.double()
    grid = torch.linspace(-40, 40, 800001, dtype=F64)
    s = torch.sigmoid(1.702 * grid)
    assert float((s * (1 + 1.702 * grid * (1 - s))).abs().max()) < 1.1  # |d/dx x sigmoid(1.702 x)|
    ref = qgelu_ref(x)
    d = K * 2.0**-23 * absacc64(A, W) + 4 * 2.0**-24 * (acc.abs() + bias.double().abs())
    tol = qgelu_tol(ref, x) + 1.1 * d
    outs = []
    for variant in (1, 3, 4):  # 394 x 384: the 256 x 256 kernel has one interior tile, the rest edge tiles
        w = f"QuickGELU random op {op} variant {variant}"
        outs.append(qlaunch(eng, op, A, W, variant, bias, w))
        assert_close(outs[-1].double(), ref, tol, w)
    assert torch.equal(outs[0].view(I16), outs[1].view(I16)) and torch.equal(outs[1].view(I16), outs[2].view(I16))
    assert_mutant_far(gelu_ref(x), ref, tol, 2000, "erf-GELU")


# ---------------------------------------------------------------------------------------------------------------------
# (2) pre_ln_rows

PRE_FAMILIES = ("normal", "offset30", "massive", "constant")


def pre_rows(d, rows):
    """`rows` bf16 rows of d from the four families of the statistics tests, and the indices of the constant ones"""
    blocks = []
    for k in range(-(-rows // 126) if rows > 5 else 1):
        X, fam = ln_rows(d, 4000 + d + k)
        blocks.append(X[:126])  # normal 0..39, offset30 40..79, massive 80..119, constant 120..125
    X = torch.cat(blocks)
    if rows == 1:
        X = X[80:81]
    elif rows == 5:
        X = X[[0, 40, 80, 120, 121]]
    X = X[:rows].contiguous()
    const = (X.double().max(1).values == X.double().min(1).values).nonzero().reshape(-1)
    return X, const


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("rows", [1, 5, 397])
@pytest.mark.parametrize("d", [384, 768, 1024])
def test_pre_ln_rows(eng, d, rows, eps):
    e32 = float(np.float32(eps))
    X, const = pre_rows(d, rows)
    assert X.shape == (rows, d)
    g = _gen(7 + d)
    gamma, beta = (1.0 + _randn((d,), g, 0.25)).contiguous(), _randn((d,), g, 0.5)
    xb = Guard(BF16, rows, d)
    xb.valid.copy_(X)
    st = Guard(F32, rows, 2)
    eng.clip_apply("pre_ln", x=xb.view, gamma=gamma, beta=beta, stats=st.view, rows=rows, d=d, eps=eps)
    xb.check("pre_ln_rows output")  # nothing beyond `rows`
    st.check("pre_ln_rows statistics")
    got = xb.valid.clone()
    x = X.double()
    mean_ref, var_ref = stats_ref(X)
    rstd_ref = (var_ref + e32) ** -0.5
    ref = (x - mean_ref[:, None]) * rstd_ref[:, None] * gamma.double() + beta.double()
    e = d * 2.0**-23
    tol = ulp_bf16(ref) / 2 + e * ((x.abs() + mean_ref.abs()[:, None]) * rstd_ref[:, None] * gamma.double().abs() + beta.double().abs())
    assert_close(got.double(), ref, tol, f"pre_ln_rows d {d} rows {rows} eps {eps:g}")
    if const.numel():  # a constant row leaves beta, rounded
        assert_bits(got[const].view(I16), beta.to(BF16).view(I16)[None].expand(const.numel(), d), "constant rows")
    # the statistics: bit-equal to the canonical kernel on the kernel's own output
    st2 = Guard(F32, rows, 2)
    eng.rowop_apply("ln_stats_canonical", x=xb.view, stats=st2.view, row0=0, row1=rows, d=d, eps=eps)
    assert bool(torch.isfinite(st.valid).all())
    assert_bits(st.valid_bits(), st2.valid_bits(), f"pre_ln_rows statistics vs ln_stats_canonical on its output (d {d}, rows {rows})")
    # mutants
    mu_un, var_un = ref.mean(1), ((ref - ref.mean(1, keepdim=True)) ** 2).mean(1)
    st_un = torch.stack([mu_un, (var_un + e32) ** -0.5], 1).float()
    n = int((st_un.view(I32) != st.valid_bits()).any(1).sum())
    assert n >= max(1, rows * 3 // 4), f"mutant 'statistics of the unrounded values' differs on {n} of {rows} rows only"
    live = torch.ones(rows, dtype=torch.bool, device=DEV)
    live[const] = False
    swapped = (x - mean_ref[:, None]) * rstd_ref[:, None] * beta.double() + gamma.double()
    assert_mutant_far(swapped[live], ref[live], tol[live], int(live.sum()) * d // 4, "gamma and beta exchanged")
    if rows > 1:
        n = int((torch.roll(st.valid_bits(), 1, 0) != st.valid_bits()).any(1).sum())
        assert n >= rows // 2, f"mutant 'the neighbouring row's statistics' differs on {n} of {rows} rows only"


# ---------------------------------------------------------------------------------------------------------------------
# (3) pool_ln_rows, l2_rows


def ln_ref_np(x, gamma, beta, eps, dtype):
    x, gamma, beta = x.astype(dtype), gamma.astype(dtype), beta.astype(dtype)
    mean = x.mean(1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(eps)) * gamma + beta


def l2_ref_np(x, dtype):
    x = x.astype(dtype)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=dtype)), dtype(1e-12))


@pytest.mark.parametrize("d", [384, 768, 1024])
@pytest.mark.parametrize("tok", [0, 196])
@pytest.mark.parametrize("B", [1, 5])
def test_pool_ln_rows(eng, B, tok, d):
    eps = 1e-5
    rng = np.random.default_rng(900 + d + tok + B)
    xh = rng.standard_normal((B * T, d)).astype(np.float32)
    if B > 1:
        xh[1 * T + tok] += 30.0
        xh[2 * T + tok] *= 100.0
        xh[3 * T + tok] = 0.0  # zero row: beta
    gamma = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
    X = torch.from_numpy(xh).to(DEV).to(BF16)
    y = Guard(BF16, B, d)
    eng.clip_apply("pool_ln", x=X, gamma=torch.from_numpy(gamma).to(DEV), beta=torch.from_numpy(beta).to(DEV), y=y.view, B=B, tok=tok, d=d, eps=eps)
    y.check("pool_ln_rows")
    rows = X.view(B, T, d)[:, tok].float().cpu().numpy()
    e32 = float(np.float32(eps))
    ref = ln_ref_np(rows, gamma, beta, e32, np.float64)
    yard = float(np.abs(ln_ref_np(rows, gamma, beta, e32, np.float32).astype(np.float64) - ref).max())
    floor = max(8 * yard, 2.0**-22 * float(np.abs(ref).max()))
    reft = torch.from_numpy(ref).to(DEV)
    tol = ulp_bf16(reft) / 2 + floor
    print(f"pool_ln_rows B {B} tok {tok} d {d}: float32 yardstick {yard:.3g}")
    assert_close(y.valid.double(), reft, tol, f"pool_ln_rows B {B} tok {tok} d {d}")
    if B > 1:
        assert_bits(y.valid[3].view(I16)[None], torch.from_numpy(beta).to(DEV).to(BF16).view(I16)[None], "zero row: beta")
    other = X.view(B, T, d)[:, tok - 1 if tok else 1].float().cpu().numpy()
    mut = torch.from_numpy(ln_ref_np(other, gamma, beta, e32, np.float64)).to(DEV)
    assert_mutant_far(mut, reft, tol, B * d // 2, "the neighbouring token pooled")
    nrm = torch.from_numpy(l2_ref_np(ref, np.float64)).to(DEV)
    assert_mutant_far(nrm, reft, tol, B * d // 2, "an L2 step left in")


@pytest.mark.parametrize("P", [64, 256, 512, 1024])
@pytest.mark.parametrize("rows", [1, 5])
def test_l2_rows(eng, rows, P):
    rng = np.random.default_rng(300 + P + rows)
    xh = (rng.standard_normal((rows, P)) * 3.0).astype(np.float32)
    if rows > 1:
        xh[1] *= 1e-10
        xh[2] *= 1e15
        xh[3] = 0.0  # a zero row gives zeros
    X = torch.from_numpy(xh).to(DEV)
    y32, y16 = Guard(F32, rows, P), Guard(BF16, rows, P)
    eng.clip_apply("l2", xf=X, y_f32=y32.view, y_bf16=y16.view, rows=rows, p=P)
    y32.check("l2_rows f32")
    y16.check("l2_rows bf16")
    got = y32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(y16.valid_bits(), got.to(BF16).view(I16), "l2_rows: bf16 output vs RNE of the f32 output")
    ref = l2_ref_np(xh, np.float64)
    yard = float(np.abs(l2_ref_np(xh, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    print(f"l2_rows rows {rows} P {P}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol
    if rows > 1:
        assert bool((got[3] == 0).all()) and bool((y16.valid[3].float() == 0).all())
        assert np.allclose(np.linalg.norm(got.double().cpu().numpy()[[0, 1, 2, 4]], axis=1), 1.0, atol=1e-6)
    assert int((np.abs(xh.astype(np.float64) / np.maximum(np.abs(xh).sum(1, keepdims=True), 1e-12) - ref) > 4 * tol).sum()) >= (rows - (rows > 1)) * P // 2, "mutant 'L1 norm'"
    only = Guard(BF16, rows, P)
    eng.clip_apply("l2", xf=X, y_bf16=only.view, rows=rows, p=P)
    assert torch.equal(only.valid_bits(), y16.valid_bits())


# ---------------------------------------------------------------------------------------------------------------------
# (4) prepared buffers


def _as_vit_names(m, g):
    """the tower's tensors under the ViT names of tests/test_gpu_weight_prep.py's table (layer_norm1 -> layernorm_before, ...)"""
    v = "vision_model."
    o = {"embeddings.cls_token": m[v + "embeddings.class_embedding"], "embeddings.position_embeddings": m[v + "embeddings.position_embedding.weight"],
         "embeddings.patch_embeddings.projection.weight": m[v + "embeddings.patch_embedding.weight"],
         "embeddings.patch_embeddings.projection.bias": None, "layernorm.weight": m[v + "post_layernorm.weight"], "layernorm.bias": m[v + "post_layernorm.bias"]}
    for l in range(g.num_layers):
        p, q = f"{v}encoder.layers.{l}.", f"layers.{l}."
        for wb in ("weight", "bias"):
            o[q + "layernorm_before." + wb] = m[p + "layer_norm1." + wb]
            o[q + "layernorm_after." + wb] = m[p + "layer_norm2." + wb]
            for a, b in (("q_proj", "q_proj"), ("k_proj", "k_proj"), ("v_proj", "v_proj"), ("o_proj", "out_proj")):
                o[q + f"attention.{a}.{wb}"] = m[p + f"self_attn.{b}.{wb}"]
            o[q + "mlp.fc1." + wb] = m[p + "mlp.fc1." + wb]
            o[q + "mlp.fc2." + wb] = m[p + "mlp.fc2." + wb]
    return o


@pytest.mark.parametrize("case", [("bfloat16", CLIPGeometry(hidden_size=384, num_layers=2, num_heads=6, intermediate_size=128, projection_dim=192, hidden_act="gelu")),
                                  ("float16", CLIPGeometry(hidden_size=1024, num_layers=1, num_heads=16, intermediate_size=64, projection_dim=None))],
                         ids=["384x2-bf16", "1024x1-f16-noproj"])
def test_prepared_buffers(tmp_path, case):
    import test_gpu_weight_prep as wp

    dtype, geom = case
    ckpt.save_checkpoint(tmp_path, make_clip_weights(21, geom), "clip", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "clip")
    assert ck.dtype == dtype and ck.geometry == geom
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_clip_checkpoint(ck)
        host.load_clip({k: t.float().numpy() for k, t in ck.tensors.items()}, geom)
        (bd, fd), (bh, fh) = wp._read_all(dev), wp._read_all(host)
        info = dev.encoder_info()
    finally:
        dev.close()
        host.close()
    D, L = geom.hidden_size, geom.num_layers
    assert info == {"kind": "clip", "embed_dim": geom.embed_dim, "hidden_act": geom.hidden_act, "projection_dim": geom.projection_dim}
    assert len(bd) == len(bh) == 6 + 18 * L + (3 if geom.projection_dim else 2) and fd == fh
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    wp.DEV_OF[0] = DEV
    m = {k: t.to(DEV) for k, t in ck.tensors.items()}
    table = wp.vit_table(_as_vit_names(m, geom), geom)
    assert table[2][0] == "patch_b"
    table[2] = ("patch_b", "zeros", D)  # all +0.0
    table += [("pre_g", "f32", m["vision_model.pre_layrnorm.weight"]), ("pre_b", "f32", m["vision_model.pre_layrnorm.bias"])]  # identical bits
    if geom.projection_dim:
        table.append(("proj_w", "bf16", m["visual_projection.weight"]))  # one RNE
        assert bd[-1].size == geom.projection_dim * D * 2
    assert bd[2].size == 4 * D and not bd[2].any()
    folds = wp.check_table(table, bd, f"clip {dtype}")
    assert len(folds) == 2 * L
    for k, (name, (d, out)) in enumerate(folds.items()):  # the folds sit under layer_norm1 / layer_norm2
        left, right, tol, (x, xc, r, W, b) = wp.function_check(name, d, out, 200 + k, f"clip {dtype}")
        other = [dd for n, (dd, _) in folds.items() if n[:2] == name[:2] and n != name]
        gm, bt = other[0]["gamma"].double(), other[0]["beta"].double()
        assert_mutant_far((gm * xc * r + bt) @ W.T + b[None], right, tol, right.numel() // 2, f"{name}: the other LayerNorm's gamma and beta")
        pg, pb = m["vision_model.pre_layrnorm.weight"].double(), m["vision_model.pre_layrnorm.bias"].double()
        assert_mutant_far((pg * xc * r + pb) @ W.T + b[None], right, tol, right.numel() // 2, f"{name}: pre_layrnorm's gamma and beta")


# ---------------------------------------------------------------------------------------------------------------------
# (5) end to end


def _pack(arrays, device="cuda:0"):
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(arrays), dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(device), offs, hw


def _golden_crops(golden_dir):
    from PIL import Image

    man = json.load(open(os.path.join(golden_dir, "crops_manifest.json")))
    return [np.array(Image.open(os.path.join(golden_dir, "crops", c["file"])).convert("RGB")) for c in man["crops"]]


def _close_all(emb):
    for e in emb.engines:
        e.close()


@pytest.mark.parametrize("key", ["B", "S2", "L3", "B2"])
def test_end_to_end_against_the_restatement_and_transformers(golden_dir, key):
    from oracle import preprocess as opre

    geom, w = geom_of(key), weights_of(key)
    arrays = list(synthetic_crops(mk.N_CROPS, seed=mk.CROP_SEED)) + _golden_crops(golden_dir)
    assert len(arrays) == 40
    pv = np.stack([opre.preprocess_crop(a) for a in arrays]).astype(np.float32)
    emb = RegionEmbedder(device=0, encoder="clip", weights=w, geometry=geom, pool="cls", chunk=64)
    try:
        assert emb.embed_dim == geom.embed_dim and emb.engine.encoder_info()["hidden_act"] == geom.hidden_act
        pix, offs, hw = _pack(arrays)
        e32, e16 = emb.embed_packed(pix, offs, hw)
        torch.cuda.synchronize()
        assert emb.engine.attention_redone(geom.num_layers) == [0] * geom.num_layers  # no attention layer redone
        got = e32.cpu().numpy()
        assert got.shape == (40, geom.embed_dim) and tuple(e16.shape) == (40, geom.embed_dim)
        assert np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)  # the reference surface returns rows of embed_dim too
        assert rows.shape == (3, geom.embed_dim) and ok.all() and np.array_equal(rows, got[:3])
        lists = emb.get_image_embeddings(arrays[:2])
        assert [len(v) for v in lists] == [geom.embed_dim] * 2 and np.array_equal(np.array(lists, dtype=np.float32), got[:2])
        assert np.array_equal(emb.embed(arrays[16]), got[16])
    finally:
        _close_all(emb)
    want = cr.clip_embed(pv, w, geom, torch.float32, "cls")
    omc = cr.one_minus_cos(got, want)
    print(f"clip parity {key} ({geom.hidden_size}-d x {geom.num_layers} layers, {geom.hidden_act}, P {geom.projection_dim}): "
          f"max(1 - cos) = {omc.max():.3g} (synthetic 224^2: {omc[:16].max():.3g}, bundled: {omc[16:].max():.3g})")
    assert float(omc.max()) <= 1e-3, (key, float(omc.max()))
    mu = want.mean(axis=0, keepdims=True)
    a, b = got - mu, want - mu  # centred: near-identical seeded-weight embeddings cannot pass trivially
    ccos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert np.all(ccos > 0.98), (key, float(ccos.min()))
    rec = np.load(os.path.join(golden_dir, "clip_cases.npz"))[f"{key}.image_embeds" if geom.projection_dim else f"{key}.pooler_output"]
    omc_hf = cr.one_minus_cos(got[:16], rec)  # what transformers itself returned on the 224 x 224 crops (both resize rules: the identity)
    print(f"clip parity {key}: against the recorded transformers rows max(1 - cos) = {omc_hf.max():.3g}")
    assert float(omc_hf.max()) <= 1e-3, (key, float(omc_hf.max()))


@pytest.mark.parametrize("key", ["B2", "S2"])
def test_layernorm_kernel_mode_against_the_restatement(key):
    """ln_fusion 0: LayerNorm kernels and the unfolded fc1 epilogues (EPI_BIAS_QGELU for a quick_gelu tower); same bound.
    On these two-layer towers the other activation moves the embedding by 1.6e-5 / 5.5e-6 in 1 - cos only (f32 restatement), so
    this case shows that the mode runs and stays within the bound; the activation itself is held element by element in (1)."""
    from oracle import preprocess as opre

    geom, w = geom_of(key), weights_of(key)
    crops = synthetic_crops(mk.N_CROPS, seed=mk.CROP_SEED)
    pv = np.stack([opre.preprocess_crop(a) for a in crops]).astype(np.float32)
    eng = Engine(0)
    try:
        eng.load_clip(w, geom)
        eng.set_chunk(64)
        eng.set_ln_fusion(0)
        got0 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
        eng.set_ln_fusion(2)
        got2 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
    finally:
        eng.close()
    want = cr.clip_embed(pv, w, geom, torch.float32, "cls")
    omc0, omc2 = cr.one_minus_cos(got0, want), cr.one_minus_cos(got2, want)
    print(f"clip parity {key}, LayerNorm-kernel mode: max(1 - cos) = {omc0.max():.3g} (folded mode: {omc2.max():.3g})")
    assert float(omc0.max()) <= 1e-3 and float(omc2.max()) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# (6) bit identities


@pytest.fixture(scope="module")
def crops40():
    return torch.from_numpy(synthetic_crops(40, seed=3)).cuda()


def _uniform(engine, crops, pool_token=0):
    n = crops.shape[0]
    per = int(np.prod(crops.shape[1:]))
    offs = np.arange(n, dtype=np.int64) * per
    hw = np.tile(np.array([[crops.shape[1], crops.shape[2]]], dtype=np.int32), (n, 1))
    e32, e16 = engine.embed(crops.reshape(-1), offs, hw, pool_token)
    torch.cuda.synchronize()
    return e32, e16


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_checkpoint_directory_equals_weights_dict(tmp_path, crops40, dtype):
    geom, w = geom_of("S2"), weights_of("S2")
    ckpt.save_checkpoint(tmp_path, w, "clip", dtype, geometry=geom, image_mean=(0.5, 0.5, 0.5), image_std=(0.25, 0.25, 0.25),
                         image_processor_type="CLIPImageProcessor")
    by_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="clip")
    ck = by_dir.checkpoint
    by_dict = RegionEmbedder(device=0, chunk=64, encoder="clip", weights={k: t.float().numpy() for k, t in ck.tensors.items()}, geometry=geom)
    try:
        by_dict.engine.set_normalisation((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
        assert ck is not None and ck.geometry == geom and ck.dtype == dtype
        assert by_dir.embed_dim == by_dict.embed_dim == 256
        assert by_dir.engine.weights_fingerprint() == by_dict.engine.weights_fingerprint()
        a32, a16 = by_dir.embed_uniform(crops40)
        b32, b16 = by_dict.embed_uniform(crops40)
        torch.cuda.synchronize()
        assert torch.equal(a32, b32) and torch.equal(a16, b16) and bool(torch.isfinite(a32).all()) and tuple(a32.shape) == (40, 256)
    finally:
        _close_all(by_dir)
        _close_all(by_dict)


@pytest.mark.parametrize("key", ["S2", "L3"])
def test_forward_settings_are_bit_identical(crops40, key):
    geom = geom_of(key)
    eng = Engine(0)
    try:
        eng.load_clip(weights_of(key), geom)
        crops = torch.cat([crops40, torch.from_numpy(synthetic_crops(260, seed=9)).cuda()])  # 300 crops: interior 256-row tiles and a ragged one
        eng.set_chunk(300)
        eng.set_ln_fusion(1)
        ref, _ = _uniform(eng, crops)
        assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (300, geom.embed_dim)
        for variant in (0, 1, 3, 4, 6):
            eng.set_gemm_variant(variant)
            for mode in (2, 1):
                eng.set_ln_fusion(mode)
                got, _ = _uniform(eng, crops)
                assert torch.equal(ref, got), (key, "gemm variant", variant, "ln fusion", mode)
        eng.set_gemm_variant(0)
        eng.set_ln_fusion(2)
        for tok in (0, 196):
            eng.set_forward_pruning(False)
            full, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(True)
            pruned, _ = _uniform(eng, crops, tok)
            eng.set_forward_pruning(False)
            assert torch.equal(full, pruned), (key, "pruning", tok)
        eng.set_chunk(64)
        c64, _ = _uniform(eng, crops40)
        eng.set_chunk(8)
        c8, _ = _uniform(eng, crops40)
        assert torch.equal(c64, c8), (key, "chunk 64 vs 8")
        assert torch.equal(c64, ref[:40]), (key, "the same crops inside a pass of 300")
        for order in (0, 2, 1):
            eng.set_tile_order(order)
            got, _ = _uniform(eng, crops40)
            assert torch.equal(got, c8), (key, "tile order", order)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (7) one context: ViT-B seeds -> CLIP -> the same ViT-B seeds


def test_vit_then_clip_then_vit_on_one_context(crops40):
    vg = dataclasses.replace(VIT_B16, num_layers=2)  # ViT-B/16 width, two layers: the load sequence is the same at any depth
    vw = make_vit_weights(5, vg)
    fresh = Engine(0)
    try:
        fresh.load_clip(weights_of("B2P"), B2P)
        fresh.set_chunk(64)
        clip_solo = [t.clone() for t in _uniform(fresh, crops40)]
        clip_fp = fresh.weights_fingerprint()
    finally:
        fresh.close()
    e = Engine(0)
    try:
        e.set_chunk(64)
        assert e.encoder_info() == {"kind": "vit", "embed_dim": 768, "hidden_act": "gelu", "projection_dim": None}
        e.load_vit(vw, geom=vg)
        first = [t.clone() for t in _uniform(e, crops40)]
        vit_fp = e.weights_fingerprint()
        assert e.embed_dim == 768 and len(vit_fp) == 6 + 18 * 2
        e.load_clip(weights_of("B2P"), B2P)
        assert e.encoder_info() == {"kind": "clip", "embed_dim": 512, "hidden_act": "quick_gelu", "projection_dim": 512}
        assert e.weights_fingerprint() == clip_fp and len(clip_fp) == 6 + 18 * 2 + 3
        second = _uniform(e, crops40)
        assert tuple(second[0].shape) == (40, 512) and torch.equal(second[0], clip_solo[0]) and torch.equal(second[1], clip_solo[1])
        e.load_vit(vw, geom=vg)
        assert e.encoder_info() == {"kind": "vit", "embed_dim": 768, "hidden_act": "gelu", "projection_dim": None}
        assert e.weights_fingerprint() == vit_fp
        third = _uniform(e, crops40)
        assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
        assert not torch.equal(first[0][:, :512], second[0])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# (8) downstream at d = 512


def test_downstream_cosine_neighbours_and_page_matrix_at_512():
    from multimodal_embeddings_amd.cross_compare import cross_compare, to_unit_bf16
    from multimodal_embeddings_amd.region_compare import region_neighbours
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection
    from oracle import compare as oc

    eng = Engine(0)
    try:
        eng.load_clip(weights_of("B2P"), B2P)
        crops = torch.from_numpy(synthetic_crops(256, seed=17)).cuda()
        e32, e16 = _uniform(eng, crops)
        assert tuple(e16.shape) == (256, 512)
        rows64 = e16.float().cpu().numpy().astype(np.float64)
        sim = cross_compare(e16, engine=eng)
        assert tuple(sim.shape) == (256, 256)
        err = float(np.abs(sim.cpu().numpy().astype(np.float64) - rows64 @ rows64.T).max())
        print(f"cross_compare d 512: max |gpu - f64| = {err:.3g}")
        assert err <= 2e-6, err
        sim_np = cross_compare(e32.cpu().numpy(), engine=eng)
        assert isinstance(sim_np, np.ndarray) and np.abs(sim_np - oc.cosine_matrix(e32.cpu().numpy())).max() < 1.5e-2
        col = RegionCollection()
        ids = [f"region_{r}" for r in range(256)]
        metas = [{"parent_image": f"/data/pages/Paper {r // 16:02d}.png", "region_type": "plain_text", "box_str": "0,0,1,1",
                  "area_percentage": 1.0 + (r % 7), "is_region": True} for r in range(256)]
        col.upsert(ids=ids, embeddings=e32.cpu().numpy().tolist(), metadatas=metas)
        rep = region_neighbours(col, top_n=10, score="cosine", threshold=0.3, engine=eng)
        assert [r["id"] for r in rep] == ids
        unit = to_unit_bf16(e32.cpu().numpy(), eng)
        u64 = unit.float().cpu().numpy().astype(np.float64)
        C = eng.cosine(unit, unit).cpu().numpy()
        assert float(np.abs(C.astype(np.float64) - u64 @ u64.T).max()) <= 2e-6
        group = (np.arange(256) // 16).astype(np.int32)
        want_idx, want_sim, _ = oc.neighbour_lists(None, group, top_n=10, fetch=30, sim=C, min_sim=0.3)
        for r, entry in enumerate(rep):
            got = [int(s["id"].split("_")[1]) for s in entry["similar_regions"]]
            assert got == [int(c) for c in want_idx[r] if c >= 0], r
            assert [s["score"] for s in entry["similar_regions"]] == [float(np.float32(v)) for v, c in zip(want_sim[r], want_idx[r]) if c >= 0], r
        assert sum(len(e["similar_regions"]) for e in rep) >= 256
        # the page matrix over the same collection against the oracle's loop on the kernel's own cosine values (tests/test_gpu_pipeline.py)
        from multimodal_embeddings_amd.weighted_region_clustering import compute_image_similarity_matrix

        names = [f"Paper {p:02d}.png" for p in range(16)]
        for m in metas:
            m["parent_image_name"] = os.path.basename(m["parent_image"])
        col2 = RegionCollection()
        col2.upsert(ids=ids, embeddings=e32.cpu().numpy().tolist(), metadatas=metas)
        S, nm = compute_image_similarity_matrix(col2, ["/data/pages/" + n for n in names], engine=eng)
        area = np.array([m["area_percentage"] for m in metas], dtype=np.float64)
        S_want, _ = oc.compute_image_similarity_matrix(None, area, np.repeat(np.arange(16), 16), names, [m["region_type"] for m in metas], sim=C,
                                                       skip_same_prefix=True)
        assert nm == names and S.shape == (16, 16) and np.array_equal(np.diag(S), np.ones(16))
        assert np.abs(S - S_want).max() <= 1e-12
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (9) refusals


def test_load_clip_refusals_keep_the_previous_weights(crops40):
    geom, w = geom_of("S2"), weights_of("S2")
    eng = Engine(0)
    try:
        eng.load_clip(w, geom)
        eng.set_chunk(64)
        before = [t.clone() for t in _uniform(eng, crops40)]
        fp, info = eng.weights_fingerprint(), eng.encoder_info()
        import ctypes as C

        keep = []

        def arr(name):
            a = np.ascontiguousarray(w[name], dtype=np.float32)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(C.c_float))

        def attempt(change, pattern):
            W, layers = eng._weights_struct("clip", geom, arr)
            change(W)
            rc = eng.lib.mme_load_clip(eng.h, C.byref(W))
            text = eng.lib.mme_last_error(eng.h).decode()
            assert rc == -1 and pattern in text, (rc, text)
            assert eng.weights_fingerprint() == fp and eng.encoder_info() == info
            e32, e16 = _uniform(eng, crops40)
            assert torch.equal(e32, before[0]) and torch.equal(e16, before[1])

        attempt(lambda W: setattr(W, "proj_dim", 100), "proj_dim = 100; supported: 0 (no projection) or a multiple of 64 up to 1024")
        attempt(lambda W: setattr(W, "pre_g", None), "pre_g / pre_b (pre_layrnorm) is a null tensor pointer")
        attempt(lambda W: setattr(W, "act", 2), "act = 2; supported: 0 (erf-GELU), 1 (QuickGELU)")
        attempt(lambda W: setattr(W.vit, "hidden", 512), "mme_load_clip: hidden = 512; supported: 384, 768, 1024")
        with pytest.raises(MmeError, match="expected"):
            eng.load_clip(w, geom_of("L3"))
    finally:
        eng.close()


def test_clip_apply_refuses_bad_arguments(eng):
    d, rows, P = 768, 8, 256
    g = _gen(2)
    gamma, beta = _randn((d,), g), _randn((d,), g)
    x = Guard(BF16, rows + 1, d)
    st = Guard(F32, rows, 2)
    y = Guard(BF16, rows, d)
    yf = Guard(F32, rows + 1, P)
    xf = _randn((rows + 1, P), g)
    A, W = _randn((64 + 1, 128), g, 1.0, BF16), _randn((64, 128), g, 1.0, BF16)
    out = Guard(BF16, 64, 64)
    bias = torch.zeros(64 + 4, dtype=F32, device=DEV)
    cases = [
        (dict(op=5, x=x.view, gamma=gamma, beta=beta, stats=st.view, rows=rows, d=d), "op 5 outside 0..4"),
        (dict(op=-1, xf=xf, y_f32=yf.view, rows=rows, p=P), "op -1 outside 0..4"),
        (dict(op=2, x=x.view, gamma=gamma, beta=beta, stats=st.view, rows=rows, d=1280), "built for d == 384, d == 768 and d == 1024 (d = 1280)"),
        (dict(op=3, x=x.view, gamma=gamma, beta=beta, y=y.view, B=0, tok=0, d=1280), "(d = 1280)"),
        (dict(op=2, x=x.view.reshape(-1)[1:], gamma=gamma, beta=beta, stats=st.view, rows=rows, d=d), "16-byte aligned"),
        (dict(op=2, x=x.view, gamma=gamma, beta=beta, stats=st.view.reshape(-1)[1:], rows=rows, d=d), "stats non-null and 8-byte aligned"),
        (dict(op=2, x=x.view, gamma=gamma, beta=None, stats=st.view, rows=rows, d=d), "x, gamma, beta non-null"),
        (dict(op=3, x=x.view, gamma=gamma, beta=beta, y=y.view.reshape(-1)[1:], B=0, tok=0, d=d), "y non-null and 16-byte aligned"),
        (dict(op=3, x=x.view, gamma=gamma, beta=beta, y=y.view, B=0, tok=197, d=d), "0 <= tok <= 196"),
        (dict(op=4, xf=xf, y_f32=yf.view, rows=rows, p=100), "p = 100"),
        (dict(op=4, xf=xf, y_f32=yf.view, rows=rows, p=1088), "p = 1088"),
        (dict(op=4, xf=xf.reshape(-1)[1:], y_f32=yf.view, rows=rows, p=P), "xf non-null and 16-byte aligned"),
        (dict(op=4, xf=xf, y_f32=yf.view.reshape(-1)[1:], rows=rows, p=P), "y_f32 and y_bf16 16-byte aligned"),
        (dict(op=4, xf=xf, rows=rows, p=P), "y_f32 or y_bf16"),
        (dict(op=0), "op 0 needs gemm"),
        (dict(op=0, A=A.reshape(-1)[4 : 4 + 64 * 128].view(64, 128), W=W, bias=bias, out=out.view, ldo=out.ld), "A and W must be 16-byte aligned"),
        (dict(op=0, A=A[:64], W=W, bias=bias.reshape(-1)[1:], out=out.view, ldo=out.ld), "bias and out must be 16-byte aligned"),
        (dict(op=0, A=A[:64], W=W, K=96, bias=bias, out=out.view, ldo=out.ld), "K = 96 must be a multiple of 64"),
        (dict(op=0, A=A[:64], W=W, variant=7, bias=bias, out=out.view, ldo=out.ld), "variant 7 outside 0..6"),
        (dict(op=1, A=A[:64], W=W, bias=bias, out=out.view, ldo=out.ld), "op 1 needs ln_stats and colsum"),
    ]
    for kw, text in cases:
        op = kw.pop("op")
        with pytest.raises(MmeError) as ei:
            eng.clip_apply(op, **kw)
        assert "(-1)" in str(ei.value) and text in str(ei.value), (op, text, str(ei.value))
    for buf in (x, st, y, yf, out):
        assert buf.untouched()
    # the two older diagnostics still refuse the new codes
    with pytest.raises(MmeError, match="outside 0..6, 8"):
        eng.gemm_apply(9, A[:64], W, bias=bias, out=out.view, ldo=out.ld)
    with pytest.raises(MmeError, match="op 6 outside"):
        eng.rowop_apply(6, x=x.view, d=d)
    assert out.untouched()
