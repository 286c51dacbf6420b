"""The Mllama language tower on the GPU (csrc/mllama_lm.hip, csrc/capi_mllama.hip).

(a) Every kernel, one launch at a time (mme_mllama_apply), against float64 computed with torch from the SAME bf16 bits the
    kernel reads, element by element.  e = 2^-24 is the unit roundoff of f32.  Each bound is the output's half ulp in bf16
    (ONE rounding of the output) plus the f32 arithmetic before it:
      rmsnorm / headnorm   the sum of d squares in f32 is off by at most d e relatively in any order, rsqrt halves that; the
                           division, eps, rsqrt (2 ulp) and the two products add 16 e:  ulp/2 + |ref| (d + 16) e
      rope                 a c - b s, each product and the difference rounded (or fused):  ulp/2 + 3 e (|a c| + |b s|)
      silu_mul             exp through exp2 carries the rounding of g log2 e, (2 |g| + 2) e relatively; 1 + ., the division and the
                           product three more:  ulp/2 + |ref| (2 |g| + 8) 2 e
      pool                 f32 out, two norms of d terms:  |ref| (2 d + 64) e; the bf16 output is the f32 output rounded, bit for bit
      self_attn            a score is a sequential f32 dot of 128 products: |ds| <= 130 e (|q| . |k|) 128^-0.5 =: delta.  The
                           weights exp(s - max) / sum change by at most 2 delta_max + 8 e relatively, P . V sums i + 1 terms
                           in f32.  P is NOT rounded:  ulp/2 + (2 delta_max + (S + 16) 2 e) (P_ref . |V|)
      cross_attn           the same with the dot in the matrix pipe (f32 accumulation of 128 products), P rounded to bf16 for
                           P . V (bf16 keeps 8 significant bits: half an ulp is 2^-8 of a value at the bottom of its binade; the
                           sum runs over the unrounded P) and the keys accumulated tile after tile and split after split in
                           f32:  ulp/2 + (2^-8 + 2 delta_max + (keys + 64) 2 e) (P_ref . |V|)
    The measured maxima (error / bound) are printed (`pytest -s`).
(b) Cross-attention is bit-identical run to run and image by image against the batch (the split of the key axis depends on the
    key count alone); the whole tower is bit-identical across chunk sizes.
(c) The whole tower against transformers' fp32 rows (tests/golden/mllama_lm_cases.npz): 1 - cos <= 1e-3, the project's bound
    for a bf16 tower against fp32 transformers, on EVERY attended row (row r is pooled by a call with
    lengths r + 1: under the causal mask nothing behind r reaches it).
(d) mme_mllama_embed == mme_tile_vit_forward's hidden (as bf16, exact) + mme_mllama_lm_forward, bit for bit.
(e) load and load_as leave bit-identical buffers; refusals by message with the outputs' sentinels intact; the forward runs on
    the caller's stream (tests/stream_probes.py); RegionEmbedder(encoder="mllama") end to end.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

import mllama_lm_reference as R
from multimodal_embeddings_amd import weights as W
from test_gpu_gemm import BF16, DEV, F32, F64, SENT16, SENT32, Guard, _gen, _randn, assert_close, ulp_bf16

pytestmark = pytest.mark.gpu

E = 2.0**-24
EPS = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mllama_lm_cases.npz")


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def report(what, got64, ref, tol):
    ratio = float(((got64 - ref).abs() / tol.clamp_min(1e-300)).max())
    print(f"{what}: max error / bound = {ratio:.3f}")
    assert_close(got64, ref, tol, what)


# ---- (a) row kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 512, 4096])
def test_rmsnorm_rows(eng, d):
    g = _gen(d)
    rows = 37
    x = _randn((rows, d), g, 1.5, BF16)
    x[3] *= 2.0**-10  # a row whose mean square is of the order of eps
    x[4] *= 2.0**10
    w = 1 + 0.25 * _randn((d,), g)
    out = Guard(BF16, rows, d)
    eng.mllama_apply("rmsnorm", x=x, y=out.view, w=w, rows=rows, d=d, eps=EPS)
    out.check("rmsnorm")
    x64 = x.double()
    ref = w.double() * (x64 / torch.sqrt((x64 * x64).mean(-1, keepdim=True) + float(np.float32(EPS))))
    report(f"rmsnorm d={d}", out.valid.double(), ref, ulp_bf16(ref) / 2 + ref.abs() * (d + 16) * E)


@pytest.mark.parametrize("heads,ld,col0", [(1, 128, 0), (4, 512, 0), (32, 4096, 0), (2, 512, 256)])
def test_headnorm_rows(eng, heads, ld, col0):
    g = _gen(heads + ld)
    rows = 21
    x = _randn((rows, ld), g, 3.0, BF16)
    before = x.clone()
    w = 1 + 0.25 * _randn((128,), g)
    eng.mllama_apply("headnorm", x=x, w=w, rows=rows, heads=heads, ld=ld, col0=col0, eps=EPS)
    h64 = before[:, col0 : col0 + heads * 128].double().view(rows, heads, 128)
    ref = (w.double() * (h64 / torch.sqrt((h64 * h64).mean(-1, keepdim=True) + float(np.float32(EPS))))).view(rows, heads * 128)
    report(f"headnorm heads={heads} ld={ld}", x[:, col0 : col0 + heads * 128].double(), ref, ulp_bf16(ref) / 2 + ref.abs() * (128 + 16) * E)
    keep = torch.ones(ld, dtype=torch.bool, device=DEV)
    keep[col0 : col0 + heads * 128] = False
    assert torch.equal(x[:, keep].view(torch.int16), before[:, keep].view(torch.int16)), "headnorm wrote outside its heads"


def test_rope_positions(eng):
    """S = 128: rows at positions 0, 1, 31 and 127 (and every other) of two sequences; Q | K heads rotated, the V heads untouched"""
    g = _gen(5)
    S, n, heads, extra = 128, 2, 3, 1
    ld = (heads + extra) * 128
    cos, sin = (torch.from_numpy(t).to(DEV) for t in W.mllama_rope_tables(R.GOLDEN_BASE))
    x = _randn((n * S, ld), g, 2.0, BF16)
    before = x.clone()
    eng.mllama_apply("rope", x=x, cos=cos, sin=sin, rows=n * S, heads=heads, ld=ld, S=S)
    pos = torch.arange(n * S, device=DEV) % S
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    h = before[:, : heads * 128].double().view(n * S, heads, 128)
    a, b = h[..., :64], h[..., 64:]
    ref = torch.cat([a * c - b * s, b * c + a * s], -1).view(n * S, heads * 128)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1).view(n * S, heads * 128)
    got = x[:, : heads * 128].double()
    report("rope", got, ref, ulp_bf16(ref) / 2 + 3 * E * mag)
    for p in (0, 1, 31, 127):
        rows = (pos == p).nonzero().flatten()
        assert_close(got[rows], ref[rows], (ulp_bf16(ref) / 2 + 3 * E * mag)[rows], f"rope position {p}")
    assert torch.equal(x[pos == 0, : heads * 128].view(torch.int16), before[pos == 0, : heads * 128].view(torch.int16)), "position 0 is the identity"
    assert torch.equal(x[:, heads * 128 :].view(torch.int16), before[:, heads * 128 :].view(torch.int16)), "rope wrote the V heads"


def test_silu_mul_rows(eng):
    g = _gen(6)
    rows, I = 19, 1024
    gu = _randn((rows, 2 * I), g, 2.5, BF16)
    rowzero = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    rowzero[[2, 7]] = 1
    out = Guard(BF16, rows, I)
    eng.mllama_apply("silu_mul", x=gu, y=out.view, rowzero=rowzero, rows=rows, d=I)
    out.check("silu_mul")
    a, b = gu[:, :I].double(), gu[:, I:].double()
    ref = a / (1 + torch.exp(-a)) * b
    ref[rowzero.bool()] = 0
    report("silu_mul", out.valid.double(), ref, ulp_bf16(ref) / 2 + ref.abs() * (2 * a.abs() + 8) * 2 * E)
    assert bool((out.valid[rowzero.bool()].view(torch.int16) == 0).all()), "a zeroed row is +0 bits"
    out2 = Guard(BF16, rows, I)
    eng.mllama_apply("silu_mul", x=gu, y=out2.view, rows=rows, d=I)
    live = ~rowzero.bool()
    assert torch.equal(out2.valid[live].view(torch.int16), out.valid[live].view(torch.int16))


def test_pool_rows(eng):
    g = _gen(7)
    n, S, d = 3, 9, 512
    lengths = np.array([9, 1, 4], dtype=np.int32)
    x = _randn((n * S, d), g, 1.5, BF16)
    w = 1 + 0.25 * _randn((d,), g)
    ef, eb = Guard(F32, n, d), Guard(BF16, n, d)
    eng.mllama_apply("pool", x=x, lengths=lengths, w=w, emb_f32=ef.view, emb_bf16=eb.view, n=n, S=S, d=d, eps=EPS)
    ef.check("pool f32")
    eb.check("pool bf16")
    rows = x.double()[torch.arange(n, device=DEV) * S + torch.from_numpy(lengths).to(DEV).long() - 1]
    v = w.double() * (rows / torch.sqrt((rows * rows).mean(-1, keepdim=True) + float(np.float32(EPS))))
    ref = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    report("pool", ef.valid.double(), ref, ref.abs() * (2 * d + 64) * E + 2.0**-126)
    assert torch.equal(eb.valid.view(torch.int16), ef.valid.to(BF16).view(torch.int16)), "the bf16 embedding is the f32 one rounded"


def test_gather_rows(eng):
    g = _gen(8)
    vocab, d = 300, 512
    tok = _randn((vocab, d), g, 1.0, BF16)
    ids = np.array([0, 299, 5, 5, 17, 298, 1], dtype=np.int32)
    out = Guard(BF16, len(ids), d)
    eng.mllama_apply("gather", tok=tok, ids=ids, x=out.view, rows=len(ids), d=d, vocab=vocab)
    out.check("gather")
    assert torch.equal(out.valid.view(torch.int16), tok[torch.from_numpy(ids).long().to(DEV)].view(torch.int16))


# ---- (a) attention ------------------------------------------------------------------------------------------------------
def self_ref(qkv, lengths, n, S, H, KVH):
    ld = (H + 2 * KVH) * 128
    t = qkv.double().view(n, S, ld)
    q, k, v = t[..., : H * 128].view(n, S, H, 128), t[..., H * 128 : (H + KVH) * 128].view(n, S, KVH, 128), t[..., (H + KVH) * 128 :].view(n, S, KVH, 128)
    kv = torch.arange(H, device=DEV) // (H // KVH)
    k, v = k[:, :, kv], v[:, :, kv]
    sc = torch.einsum("bihd,bjhd->bhij", q, k) * 128**-0.5
    mag = torch.einsum("bihd,bjhd->bhij", q.abs(), k.abs()) * 128**-0.5
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool, device=DEV), 1)
    sc = sc.masked_fill(mask, float("-inf"))
    p = torch.softmax(sc, -1)
    ref = torch.einsum("bhij,bjhd->bihd", p, v)
    pv = torch.einsum("bhij,bjhd->bihd", p, v.abs())
    dmax = (130 * E * mag).masked_fill(mask, 0).amax(-1).permute(0, 2, 1)[..., None]  # [n, S, H, 1]
    tol = ulp_bf16(ref) / 2 + (2 * dmax + (S + 16) * 2 * E) * pv
    live = (torch.arange(S, device=DEV)[None, :] < torch.from_numpy(lengths).to(DEV)[:, None])[:, :, None, None]
    return (ref * live).reshape(n * S, H * 128), (tol * live).reshape(n * S, H * 128)


@pytest.mark.parametrize("S,H,KVH", [(1, 4, 2), (2, 2, 2), (9, 4, 1), (128, 8, 1), (128, 4, 2), (9, 8, 2)])
def test_self_attention(eng, S, H, KVH):
    g = _gen(S * 100 + H * 10 + KVH)
    n = 3
    lengths = np.array([S, max(1, S // 2), 1], dtype=np.int32)  # len == S, len < S, one token
    qkv = _randn((n * S, (H + 2 * KVH) * 128), g, 1.0, BF16)
    qkv[:, : H * 128] *= 2.0  # logits of a few units
    out = Guard(BF16, n * S, H * 128)
    eng.mllama_apply("self_attn", x=qkv, y=out.view, lengths=lengths, n=n, S=S, heads=H, kv_heads=KVH)
    out.check("self_attn")
    ref, tol = self_ref(qkv, lengths, n, S, H, KVH)
    report(f"self_attn S={S} H={H} KVH={KVH}", out.valid.double(), ref, tol)
    dead = torch.from_numpy(np.concatenate([np.arange(S) >= L for L in lengths])).to(DEV)
    assert bool((out.valid[dead].view(torch.int16) == 0).all()), "rows at or behind len are +0 bits"


def cross_ref(q, kv, bits, n, S, H, KVH, T, P):
    Nk = T * P
    qd = q.double().view(n, S, H, 128)
    t = kv.double().view(n, Nk, 2 * KVH * 128)
    k, v = t[..., : KVH * 128].view(n, Nk, KVH, 128), t[..., KVH * 128 :].view(n, Nk, KVH, 128)
    sel = torch.arange(H, device=DEV) // (H // KVH)
    k, v = k[:, :, sel], v[:, :, sel]
    sc = torch.einsum("bihd,bjhd->bhij", qd, k) * 128**-0.5
    mag = torch.einsum("bihd,bjhd->bhij", qd.abs(), k.abs()) * 128**-0.5
    b = torch.from_numpy(bits.astype(np.int64)).to(DEV).view(n, S)
    b = torch.where(b == 0, torch.full_like(b, (1 << T) - 1), b)  # a row that attends no tile attends every key
    tile = torch.arange(Nk, device=DEV) // P
    allowed = ((b[:, :, None] >> tile[None, None, :]) & 1).bool()[:, None]  # [n, 1, S, Nk]
    sc = sc.masked_fill(~allowed, float("-inf"))
    p = torch.softmax(sc, -1)
    ref = torch.einsum("bhij,bjhd->bihd", p, v)
    pv = torch.einsum("bhij,bjhd->bihd", p, v.abs())
    dmax = (130 * E * mag).masked_fill(~allowed, 0).amax(-1).permute(0, 2, 1)[..., None]
    tol = ulp_bf16(ref) / 2 + (2.0**-8 + 2 * dmax + (Nk + 64) * 2 * E) * pv
    return ref.reshape(n * S, H * 128), tol.reshape(n * S, H * 128)


def mask_bits(kind, n, S, T, rng):
    if kind == "all":
        return np.full((n, S), (1 << T) - 1, dtype=np.uint8)
    if kind == "prefix":  # the processor's shape: every row the first tiles of its image
        return np.repeat(((1 << rng.integers(1, T + 1, size=n)) - 1).astype(np.uint8)[:, None], S, 1)
    if kind == "per_row":  # another non-empty set for every row
        return rng.integers(1, 1 << T, size=(n, S)).astype(np.uint8)
    bits = np.repeat(((1 << rng.integers(1, T + 1, size=n)) - 1).astype(np.uint8)[:, None], S, 1)  # "masked_row"
    bits[:, 0] = 0  # the BOS row in front of the image token
    if S > 4:
        bits[:, 3] = 0
    return bits


CROSS = [  # (S, H, KVH, T, P, mask): keys 1, 10, 148 (4 tiles + 20 keys of a fifth), 6404 (12 splits + 260 keys)
    (1, 4, 2, 1, 1, "all"), (9, 4, 2, 2, 5, "prefix"), (9, 4, 4, 3, 5, "per_row"), (9, 8, 1, 4, 37, "masked_row"), (128, 4, 2, 4, 37, "per_row"),
    (1, 2, 1, 3, 37, "masked_row"), (128, 8, 2, 2, 5, "masked_row"), (9, 4, 2, 4, 1, "prefix"), (9, 4, 2, 1, 37, "all"),
    (9, 4, 2, 4, 1601, "masked_row"),
]


@pytest.mark.parametrize("S,H,KVH,T,P,mask", CROSS)
def test_cross_attention(eng, S, H, KVH, T, P, mask):
    g = _gen(S + 7 * H + 31 * T + P)
    rng = np.random.default_rng(S + P)
    n = 1 if P == 1601 else 3
    q = _randn((n * S, H * 128), g, 1.0, BF16)
    kv = _randn((n * T * P, 2 * KVH * 128), g, 1.0, BF16)
    kv[:, : KVH * 128] *= 2.0
    bits = mask_bits(mask, n, S, T, rng)
    out = Guard(BF16, n * S, H * 128)
    args = dict(x=q, kv=kv, xmask=bits, n=n, S=S, heads=H, kv_heads=KVH, tiles=T, tokens=P)
    eng.mllama_apply("cross_attn", y=out.view, **args)
    out.check("cross_attn")
    ref, tol = cross_ref(q, kv, bits, n, S, H, KVH, T, P)
    report(f"cross_attn S={S} H={H}/{KVH} keys={T}x{P} {mask}", out.valid.double(), ref, tol)
    # (b) the same bits on a second run, and image by image
    again = Guard(BF16, n * S, H * 128)
    eng.mllama_apply("cross_attn", y=again.view, **args)
    assert torch.equal(again.valid.view(torch.int16), out.valid.view(torch.int16)), "cross_attn differs run to run"
    for b in range(n):
        one = Guard(BF16, S, H * 128)
        eng.mllama_apply("cross_attn", x=q[b * S : (b + 1) * S], kv=kv[b * T * P : (b + 1) * T * P], xmask=bits[b : b + 1], y=one.view, n=1, S=S, heads=H,
                         kv_heads=KVH, tiles=T, tokens=P)
        assert torch.equal(one.valid.view(torch.int16), out.valid[b * S : (b + 1) * S].view(torch.int16)), f"image {b} alone differs from the batch"


# ---- (c) the whole tower ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def towers():
    made = {}

    def get(name):
        if name not in made:
            from multimodal_embeddings_amd._lib import Engine

            w, geom = R.golden_tower(name)
            e = Engine(0)
            e.load_mllama_lm(w, geom)
            made[name] = (e, w, geom)
        return made[name]

    yield get
    for e, _, _ in made.values():
        e.close()


def case_inputs(z, case):
    ids, lens = z[case + ".ids"], z[case + ".lengths"]
    if case + ".vision" not in z:
        return ids, lens, None, None, None
    vis = torch.from_numpy(z[case + ".vision"]).to(DEV).to(BF16)
    return ids, lens, vis, z[case + ".num_tiles"], z[case + ".xmask"]


@pytest.mark.parametrize("case", sorted(R.GOLDEN_CASES))
def test_tower_against_transformers(towers, golden, case):
    e, w, geom = towers(R.GOLDEN_CASES[case])
    ids, lens, vis, nt, xm = case_inputs(golden, case)
    gold = golden[case + ".hidden"].astype(np.float64)
    n, S = ids.shape
    worst = 0.0
    for r in range(int(lens.max())):
        e32, e16 = e.mllama_lm_forward(ids, np.full(n, r + 1, dtype=np.int32), vision=vis, num_tiles=nt)  # the processor's rule makes the mask
        got = e32.double().cpu().numpy()
        assert np.allclose(np.linalg.norm(got, axis=-1), 1.0, atol=1e-5)
        assert torch.equal(e16.view(torch.int16), e32.to(BF16).view(torch.int16))
        for b in range(n):
            if r < lens[b]:
                row = gold[b, r] / np.linalg.norm(gold[b, r])
                worst = max(worst, 1.0 - float(got[b] @ row))
    print(f"tower {case}: max 1 - cos over the attended rows = {worst:.3e}")
    assert worst <= 1e-3
    if xm is not None:  # the caller's mask bits give the same bits as the processor's rule
        a, _ = e.mllama_lm_forward(ids, lens, vision=vis, num_tiles=nt)
        b, _ = e.mllama_lm_forward(ids, lens, vision=vis, xmask=xm)
        assert torch.equal(a, b)


def test_tower_identical_across_chunks(towers, golden):
    e, w, geom = towers("a")
    ids, lens, vis, nt, xm = case_inputs(golden, "bos_first")
    outs = []
    for chunk in (64, 1, 2):
        e.set_chunk(chunk)
        outs.append(e.mllama_lm_forward(ids, lens, vision=vis, num_tiles=nt)[0].clone())
    e.set_chunk(64)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    tids, tlens, *_ = case_inputs(golden, "text_only")
    a = e.mllama_lm_forward(tids, tlens)[0].clone()
    e.set_chunk(1)
    b = e.mllama_lm_forward(tids, tlens)[0].clone()
    e.set_chunk(64)
    assert torch.equal(a, b)


def test_info_and_coexistence(towers):
    e, w, geom = towers("a")
    info = e.mllama_lm_info()
    assert info["loaded"] and (info["hidden_size"], info["num_heads"], info["num_kv_heads"], info["num_layers"], info["num_cross_layers"]) == (512, 4, 2, 3, 1)
    assert (info["vocab_size"], info["vision_output_dim"], info["image_token_id"], info["rope_type"]) == (300, 64, 300, 1)


def test_load_and_load_as_leave_the_same_buffers(towers):
    from multimodal_embeddings_amd._lib import Engine

    e, w, geom = towers("a")
    for dtype_id, tdt in ((0, torch.float32), (1, torch.bfloat16)):  # the seeded values are bf16-representable: both stage the same values
        o = Engine(0)
        try:
            o.load_mllama_lm_tensors({k: torch.from_numpy(np.ascontiguousarray(v)).to(tdt).contiguous() for k, v in w.items()}, geom, dtype_id)
            fa, fb = e.weights_fingerprint(), o.weights_fingerprint()
            assert len(fa) == len(fb) == 7 + 6 * 2 + 9
            for i in range(len(fa)):
                assert np.array_equal(e.weights_read(i), o.weights_read(i)), f"prepared buffer {i} differs (dtype {dtype_id})"
        finally:
            o.close()


def test_a_checkpoint_directory_loads_to_the_same_buffers(towers, golden, tmp_path):
    from multimodal_embeddings_amd import checkpoint as ckpt
    from multimodal_embeddings_amd._lib import Engine

    e, w, geom = towers("a")
    ck = ckpt.read_checkpoint(ckpt.save_checkpoint(str(tmp_path / "lm"), w, "mllama_text", "bfloat16", geometry=geom), "mllama_text")
    o = Engine(0)
    try:
        o.load_mllama_lm_checkpoint(ck)
        assert o.weights_fingerprint() == e.weights_fingerprint() and o.mllama_lm_info() == e.mllama_lm_info()
        ids, lens, vis, nt, xm = case_inputs(golden, "two_lengths")
        assert torch.equal(o.mllama_lm_forward(ids, lens, vision=vis, num_tiles=nt)[0], e.mllama_lm_forward(ids, lens, vision=vis, num_tiles=nt)[0])
    finally:
        o.close()


# ---- (d) pixels to vectors ------------------------------------------------------------------------------------------------
def test_embed_equals_tile_tower_plus_language_tower():
    """Two intermediate states: with one, the feature order 1280 + d ni + k of the gathered states could not be told from 1280 + k 1280 + d."""
    from multimodal_embeddings_amd._lib import Engine

    tile = dataclasses.replace(W.TILE_VIT, num_layers=2, num_global_layers=1, intermediate_layers=(0, 1))
    geom = dataclasses.replace(R.GOLDEN_BASE, vision_output_dim=tile.output_dim)
    e = Engine(0)
    try:
        e.load_tile_vit(W.make_tile_vit_weights(2, tile), tile)
        e.load_mllama_lm(W.make_mllama_lm_weights(9, geom), geom)
        pv = _randn((1, 4, 3, 560, 560), _gen(3), 1.0, F32)
        pv[:, 2:] = 0
        aid, nt = np.array([2], dtype=np.int32), np.array([2], dtype=np.int32)
        ids = np.array([[1, 300, 1, 20, 21, 22, 23]], dtype=np.int32)
        a32, a16 = e.mllama_embed(pv, aid, nt, ids)
        hidden, _, _ = e.tile_vit_forward(pv, aid, nt, want_hidden=True, want_f32=False, want_bf16=False)
        vis = hidden.to(BF16)
        assert torch.equal(vis.float(), hidden), "the tile tower's states are bf16 values"
        b32, b16 = e.mllama_lm_forward(ids, vision=vis, num_tiles=nt)
        assert torch.equal(a32, b32) and torch.equal(a16.view(torch.int16), b16.view(torch.int16))
        assert bool(torch.isfinite(a32).all()) and abs(float(a32.norm()) - 1.0) < 1e-5
    finally:
        e.close()


# ---- (e) refusals, streams, the embedder ------------------------------------------------------------------------------------
def test_refusals_by_message(towers, golden):
    from multimodal_embeddings_amd._lib import Engine, MmeError

    e, w, geom = towers("a")
    bad = [
        (dict(num_heads=3), "hidden = 512 at heads = 3"),
        (dict(num_kv_heads=3), "kv_heads = 3 at heads = 4"),
        (dict(intermediate_size=1000), "intermediate = 1000"),
        (dict(num_layers=65), "layers = 65"),
        (dict(vocab_size=1 << 18), "vocab = 262144"),
        (dict(vision_output_dim=100), "vision_dim = 100"),
        (dict(hidden_act="gelu"), "hidden_act = -1"),
        (dict(rope_type="yarn"), "rope_type = -1"),
    ]
    before = e.weights_fingerprint()
    for change, text in bad:
        g2 = dataclasses.replace(geom, **change)
        arr = lambda name: None  # noqa: E731  (the geometry is refused before any tensor is read)
        Wst, layers = Engine._mllama_lm_struct(dataclasses.replace(g2, num_layers=min(g2.num_layers, 3)), lambda name: e_ptr(w, name), lambda name: 0.5)
        Wst.layers = g2.num_layers
        import ctypes

        rc = e.lib.mme_load_mllama_lm(e.h, ctypes.byref(Wst))
        msg = e.lib.mme_last_error(e.h).decode()
        assert rc != 0 and text in msg and "supported" in msg, (change, msg)
    assert e.weights_fingerprint() == before and e.mllama_lm_info()["loaded"], "a refused load changed the context"
    ids, lens, vis, nt, xm = case_inputs(golden, "bos_first")
    n, S = ids.shape
    out = Guard(F32, n, 512)

    def refused(text, **over):
        kw = dict(ids=ids, lens=lens, S=S, vision=vis, tiles=4, tokens=5, nt=nt, xm=None)
        kw.update(over)
        idsv, lensv = np.ascontiguousarray(kw["ids"], dtype=np.int32), np.ascontiguousarray(kw["lens"], dtype=np.int32)
        rc = e.lib.mme_mllama_lm_forward(e.h, idsv.ctypes.data, lensv.ctypes.data, n, kw["S"], None if kw["vision"] is None else kw["vision"].data_ptr(), kw["tiles"],
                                         kw["tokens"], None if kw["nt"] is None else kw["nt"].ctypes.data, None if kw["xm"] is None else kw["xm"].ctypes.data,
                                         out.view.data_ptr(), None, None)
        msg = e.lib.mme_last_error(e.h).decode()
        assert rc != 0 and text in msg, (text, msg)
        torch.cuda.synchronize()
        assert out.untouched(), f"{text}: the output was written"

    noimg = ids.copy()
    noimg[1, 1] = 5
    refused("holds no image_token_id = 300", ids=noimg)
    big = ids.copy()
    big[2, 3] = 308
    refused("id = 308", ids=big)
    refused("len = 0", lens=np.array([8, 0, 8]))
    refused("len = 9", lens=np.array([8, 9, 8]))
    refused("S = 129", S=129)
    refused("tiles = 5", tiles=5)
    refused("tokens = 1602", tokens=1602)
    refused("has 5 tiles", nt=np.array([1, 5, 4], dtype=np.int32))
    refused("mask bits = 0x10", xm=np.full((n, S), 16, dtype=np.uint8))
    with pytest.raises(MmeError, match="heads / kv_heads"):
        eng_apply_bad(e)


def e_ptr(w, name):
    import ctypes

    a = np.ascontiguousarray(w[name], dtype=np.float32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


_KEEP = []


def eng_apply_bad(e):
    q = torch.zeros((4, 3 * 128), dtype=BF16, device=DEV)
    e.mllama_apply("cross_attn", x=q, kv=q, y=q, xmask=np.ones(4, dtype=np.uint8), n=1, S=4, heads=3, kv_heads=2, tiles=1, tokens=1)


def test_forward_runs_on_the_callers_stream(golden):
    import stream_probes as SP
    from multimodal_embeddings_amd._lib import Engine

    w, geom = R.golden_tower("a")
    z = golden

    def setup():
        e = Engine(0)
        e.load_mllama_lm(w, geom)
        return e

    def inputs(v):
        ids = z["bos_first.ids"].copy()
        ids[:, 3:] = (ids[:, 3:] + 11 * v) % 290 + 3
        vis = torch.from_numpy(z["bos_first.vision"]).to(BF16)
        vis = torch.roll(vis, v, 0) if v else vis
        return {"vision": vis}, {"ids": ids, "lengths": z["bos_first.lengths"].copy(), "num_tiles": np.roll(z["bos_first.num_tiles"], v).copy()}

    def call(e, dev, host):
        e32, e16 = e.mllama_lm_forward(host["ids"], host["lengths"], vision=dev["vision"], num_tiles=host["num_tiles"])
        return {"e32": e32, "e16": e16}

    case = SP.Case("mme_mllama_lm_forward", "mllama_lm_forward", setup, inputs, call)
    bad, effective = SP.probe_a(case)
    assert not bad, bad
    bad, effective = SP.probe_b(case)
    assert not bad, bad


def test_the_librarys_rotary_tables_are_the_python_ones(towers):
    """Prepared buffers 5 and 6 of the tower (cos, sin, built by the library's host code) against weights.mllama_rope_tables.  The two
    form inv_freq with different pow routines: 2^-20 relatively (the bound of tests/test_mllama_lm_cpu.py's comparison with transformers);
    the angle pos * inv_freq carries that and its own f32 rounding, and |d cos|, |d sin| <= |d angle|; + one rounding of the result."""
    for name in ("a", "b"):
        e, w, geom = towers(name)
        first = e.mllama_lm_info()["first_buffer"]
        want = W.mllama_rope_tables(geom)
        angle = np.arange(128, dtype=np.float64)[:, None] * W.mllama_rope_inv_freq(geom).astype(np.float64)[None, :]
        tol = angle * (2.0**-20 + 2.0**-24) + 2.0**-24
        for k in (0, 1):
            got = e.weights_read(first + 5 + k).view(np.float32).reshape(128, 64)
            err = np.abs(got.astype(np.float64) - want[k].astype(np.float64))
            print(f"rotary table {name}[{k}]: max error / bound = {(err / tol).max():.3f}")
            assert np.all(err <= tol)
        assert np.all(e.weights_read(first + 5).view(np.float32)[:64] == 1) and np.all(e.weights_read(first + 6).view(np.float32)[:64] == 0)


def test_embed_and_load_as_run_on_the_callers_stream():
    """mme_mllama_embed (tile tower pass, gather, projector, staging, language tower) and mme_load_mllama_lm_as under the probes."""
    import stream_probes as SP
    from multimodal_embeddings_amd._lib import Engine

    tile = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
    geom = dataclasses.replace(R.GOLDEN_BASE, vision_output_dim=tile.output_dim)
    tw, lw = W.make_tile_vit_weights(2, tile), W.make_mllama_lm_weights(9, geom)
    host = {k: torch.from_numpy(np.ascontiguousarray(v)).to(BF16).contiguous() for k, v in lw.items()}

    def setup():
        e = Engine(0)
        e.load_tile_vit(tw, tile)
        e.load_mllama_lm(lw, geom)
        return e

    def inputs(v):
        pv = torch.randn((1, 4, 3, 560, 560), generator=torch.Generator().manual_seed(20 + v))
        pv[:, 2:] = 0
        ids = np.array([[1, 300, 1, 20 + v, 21, 22 + 2 * v, 23]], dtype=np.int32)
        return {"pv": pv}, {"aid": np.array([2], dtype=np.int32), "nt": np.array([2], dtype=np.int32), "ids": ids, "lengths": np.array([7 - v % 2], dtype=np.int32)}

    def call(e, dev, h):
        e32, e16 = e.mllama_embed(dev["pv"], h["aid"], h["nt"], h["ids"], h["lengths"])
        return {"e32": e32, "e16": e16}

    case = SP.Case("mme_mllama_embed", "mllama_embed", setup, inputs, call)
    for probe in (SP.probe_a, SP.probe_b):
        bad, effective = probe(case)
        assert not bad, (probe.__name__, bad)

    def inputs_as(v):
        vis = torch.randn((1, 2, 5, tile.output_dim), generator=torch.Generator().manual_seed(30 + v)).to(BF16)
        return {"vision": vis}, {"ids": np.array([[1, 300, 1, 20 + v, 21]], dtype=np.int32), "nt": np.array([2], dtype=np.int32)}

    def call_as(e, dev, h):
        e.load_mllama_lm_tensors(host, geom, 1)  # prepared on the caller's stream; the forward behind it reads the buffers on that stream
        e32, _ = e.mllama_lm_forward(h["ids"], vision=dev["vision"], num_tiles=h["nt"], want_bf16=False)
        return {"e32": e32}

    case = SP.Case("mme_load_mllama_lm_as", "load_mllama_lm_as", lambda: Engine(0), inputs_as, call_as)  # the load itself is the probed call
    for probe in (SP.probe_a, SP.probe_b):
        bad, effective = probe(case)
        assert not bad, (probe.__name__, bad)


def test_embed_refuses_a_bad_image_before_any_chunk_is_written():
    from multimodal_embeddings_amd._lib import Engine

    tile = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
    geom = dataclasses.replace(R.GOLDEN_BASE, vision_output_dim=tile.output_dim)
    e = Engine(0)
    try:
        e.load_tile_vit(W.make_tile_vit_weights(2, tile), tile)
        e.load_mllama_lm(W.make_mllama_lm_weights(9, geom), geom)
        e.set_chunk(1)  # the bad image is in the second chunk
        pv = torch.zeros((2, 4, 3, 560, 560), device=DEV)
        ids = np.array([[1, 300, 1, 20]] * 2, dtype=np.int32)
        out = Guard(F32, 2, 512)
        for aid, nt, text in (([1, 9], [1, 1], "image 1 has aspect-ratio id 9"), ([1, 1], [1, 5], "image 1 has aspect-ratio id 1 / 5 tiles")):
            aid, nt, lens = np.array(aid, dtype=np.int32), np.array(nt, dtype=np.int32), np.array([4, 4], dtype=np.int32)
            rc = e.lib.mme_mllama_embed(e.h, pv.data_ptr(), aid.ctypes.data, nt.ctypes.data, 2, ids.ctypes.data, lens.ctypes.data, 4, None, out.view.data_ptr(), None, None)
            msg = e.lib.mme_last_error(e.h).decode()
            torch.cuda.synchronize()
            assert rc != 0 and text in msg and out.untouched(), msg
    finally:
        e.close()


def test_region_embedder_mllama_end_to_end():
    from PIL import Image

    from multimodal_embeddings_amd.embedder import RegionEmbedder

    tile = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
    geom = dataclasses.replace(R.GOLDEN_BASE, vision_output_dim=tile.output_dim)
    prompt = [1, 300, 1, 20, 21, 22, 23]
    emb = RegionEmbedder(encoder="mllama", geometry=tile, lm_geometry=geom, prompt_ids=prompt)
    assert emb.embed_dim == 512
    names = sorted(os.listdir(os.path.join(os.path.dirname(GOLDEN), "crops")))
    crops = [Image.open(os.path.join(os.path.dirname(GOLDEN), "crops", names[0])).convert("RGB"), None,  # two bundled crops around a hole
             Image.open(os.path.join(os.path.dirname(GOLDEN), "crops", names[2])).convert("RGB")]
    got = emb.get_image_embeddings(crops)
    assert got[1] is None and got[0] is not None and got[2] is not None
    a, c = (np.asarray(torch.as_tensor(v).float().cpu()).reshape(-1) for v in (got[0], got[2]))
    assert a.shape == c.shape == (512,) and abs(np.linalg.norm(a) - 1) < 1e-2 and not np.allclose(a, c)
    t = emb.get_text_embeddings([[1, 20, 21, 22], [1, 40, 41, 42, 43, 44]])
    t = np.asarray(torch.as_tensor(t).float().cpu())
    assert t.shape == (2, 512) and np.allclose(np.linalg.norm(t, axis=-1), 1, atol=1e-2)
    with pytest.raises(ValueError, match="prompt_ids"):
        emb.get_text_embeddings("a sentence")
