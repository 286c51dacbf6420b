"""DINOv2 ViT/14 @224 image towers on the GPU (patch 14, 16 x 16 patches, 257 tokens, LayerScale folded at load).

(1) the kernels the geometry adds, one launch each (mme_dinov2_apply) on a bare context: retile_patches_p14 and embed_rows at
    257 tokens bit for bit, the row-scaled preparer bit for bit;
(2) the 257-token attention kernel against the float64 reference of tests/test_gpu_attention.py's kind, on planted bf16
    Q / K / V, every element of every row compared.  Tolerance: that file's 2^-8 |ref| + 2^-8 A (A = sum p |v| / sum p), whose
    derivation rests on the same two rounding points -- P to bf16 before P.V, the output to bf16.  Named mutants (a
    plausible kernel bug written as a change of the reference's scores) must leave 4 x the tolerance on the planted rows;
(3) the prepared buffers: device and host preparer equal, LayerScale folded as the float64 product rounded once;
(4) the whole path against the f32 restatement of tests/dinov2_reference.py and against what transformers' Dinov2Model
    returned (tests/golden/dinov2_cases.npz), max(1 - cos) <= 1e-3, the project's bound for the bf16 path (what that bound cannot see
    on std 0.02 weights -- uniform attention, Q and K exchanged, a dropped key -- is held by tests/test_gpu_tower_sharpness.py);
(5) bit identities: ln_mode 1 = 2, every GEMM variant, pruned = unpruned, chunking, tile order, embed = preprocess + forward,
    checkpoint directory = weight dict.  ln_mode 0 (the LayerNorm kernel in front of unfolded weights) rounds at other
    points than the folded modes by construction, as for every other tower; it is held to the restatement;
(6) a CLIP-B/16 load, a DINOv2 load and a CLIP-B/16 load on one context.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import dinov2_reference as dr  # noqa: E402
import make_dinov2_golden as mkd  # noqa: E402
from test_gpu_clip import _golden_crops, _pack, _uniform  # noqa: E402
from test_gpu_gemm import BF16, DEV, F32, SENT16, Guard, _gen, _randn, assert_bits, assert_close, assert_mutant_bits, assert_mutant_far  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, DINOV2_B14, make_clip_weights, make_dinov2_weights,  # noqa: E402
                                               round_to_bf16, synthetic_crops)

pytestmark = pytest.mark.gpu

I16 = torch.int16
T, NP, DH, KP = 257, 256, 64, 640
CASES = mkd.CASES
POS = "embeddings.position_embeddings"
_weights = {}
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


def weights_of(key):
    if key not in _weights:
        seed, geom, grid = CASES[key]
        _weights[key] = make_dinov2_weights(seed, geom, pos_grid=grid)
    return _weights[key]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def crops40():
    return torch.from_numpy(synthetic_crops(40, seed=3)).cuda()


def _close_all(emb):
    for e in emb.engines:
        e.close()


TINY = dataclasses.replace(DINOV2_B14, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=64)


# ---------------------------------------------------------------------------------------------------------------------
# (1) retile_patches_p14, embed_rows at 257 tokens


@pytest.mark.parametrize("rule", ["fit_pad", "clip"])
def test_retile_is_the_mapping_bit_for_bit(eng, rule):
    """What K1 writes for crops of 224 x 224, 37 x 501 and 640 x 90 under both resize rules (a patch-16 context's
    mme_preprocess), then ONE launch of the gather into a destination filled with NaN between sentinel crops: every value
    equals the numpy mapping's, columns 588..639 are zero, the crops before and after stay as they are.  A patch-14
    context's own mme_preprocess writes the same matrix."""
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(224, 224, 3), (37, 501, 3), (640, 90, 3)]]
    n = len(arrays)
    pix, offs, hw = _pack(arrays)
    e16, e14 = Engine(0), Engine(0)
    try:
        e14.load_dinov2(make_dinov2_weights(2, TINY), geom=TINY)
        assert e14.vit_geometry().patch_size == 14 and e14.vit_geometry().seq_len == T and e16.vit_geometry().patch_size == 16
        for e in (e16, e14):
            e.set_resize_rule(rule)
            e.set_chunk(2)  # two chunks: the staging buffer is reused
        p16 = e16.preprocess(pix, offs, hw)
        p14 = e14.preprocess(pix, offs, hw)
        torch.cuda.synchronize()
    finally:
        e16.close()
        e14.close()
    assert tuple(p16.shape) == (n * 196, 768) and tuple(p14.shape) == (n * NP, KP)
    want = torch.from_numpy(dr.retile_p14_reference(p16.view(I16).cpu().numpy())).to(DEV)
    dst = Guard(BF16, n * NP, KP, guard=NP)  # guard = one whole crop of sentinel rows on either side
    dst.view.fill_(float("nan"))
    eng.dinov2_apply("retile", src=p16, dst=dst.view, n=n)
    dst.check(f"retile {rule}: the rows of the crops before and after")
    got = dst.valid_bits()
    assert_bits(got, want, f"retile {rule}")
    assert bool((got[:, 588:] == 0).all()) and bool((want[:, :588] != 0).any())
    assert_bits(p14.view(I16), want, f"mme_preprocess under a patch-14 context, {rule}")
    # the mapping moves every patch: the patch-16 bytes read as [n * 256, 588] are not it; a transposed patch grid is not it either
    flat = p16.view(I16).reshape(n * NP, 588)
    assert_mutant_bits(flat, want[:, :588], n * NP * 588 // 2, "no permutation")
    t_grid = want.view(n, 16, 16, KP).transpose(1, 2).reshape(n * NP, KP)
    assert_mutant_bits(t_grid, want, n * NP * 588 // 4, "patch grid transposed")


@pytest.mark.parametrize("d", [384, 1024])
def test_embed_rows_t257_bit_for_bit(eng, d):
    n = 3
    g = _gen(70 + d)
    acc, bias = _randn((n * NP, d), g, 3.0), _randn((d,), g)
    pos, cls = _randn((T, d), g), _randn((d,), g)
    x = Guard(BF16, n * T, d)
    eng.dinov2_apply("embed_rows", acc=acc, bias=bias, pos=pos, cls=cls, x=x.view, n=n, d=d)
    x.check("embed_rows_t257")
    a, b, p, c = (t.cpu().numpy() for t in (acc, bias, pos, cls))
    want32 = np.empty((n, T, d), dtype=np.float32)
    want32[:, 1:] = (a.reshape(n, NP, d) + b[None, None]) + p[None, 1:]  # numpy float32: (acc + bias) + pos, IEEE additions
    want32[:, 0] = c + p[0]
    want = torch.from_numpy(want32.reshape(n * T, d)).to(DEV).to(BF16).view(I16)  # round to nearest even
    rows = x.valid_bits()
    clsr = torch.arange(n, device=DEV) * T
    assert_bits(rows[clsr], want[clsr], f"embed_rows_t257 d {d}: the [CLS] rows")
    assert_bits(rows, want, f"embed_rows_t257 d {d}")
    mut = want32.copy()
    mut[:, 1:] = (a.reshape(n, NP, d) + b[None, None]) + p[None, :-1]  # the position row of the patch before
    assert_mutant_bits(torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16), want, n * NP * d // 2, "pos[p] for pos[1 + p]")
    mut = want32.copy()
    mut[:, 0] = c + p[1]
    assert_mutant_bits(torch.from_numpy(mut.reshape(n * T, d)).to(DEV).to(BF16).view(I16), want, n * d // 2, "pos[1] for pos[0]")


@pytest.mark.parametrize("dt, tdt", [(0, torch.float32), (1, torch.bfloat16), (2, torch.float16)])
def test_rowscale_and_mul_single_launches(eng, dt, tdt):
    """bf16_rne(f32(factor[r] * w[r, k])) and f32(factor[r] * b[r]) against numpy float32 (one IEEE multiplication, one rounding
    to nearest even), on values that are NOT bf16-representable for the f32 case; a row-major / column-major slip is caught."""
    rows, cols = 192, 328  # cols a multiple of 8, no multiple of 64; more chunks than one block
    g = _gen(900 + dt)
    w = _randn((rows, cols), g, 0.05).to(tdt)
    f = (_randn((rows,), g, 0.5) + 1.0).to(tdt)
    b = _randn((rows,), g, 0.1).to(tdt)
    out = Guard(BF16, rows, cols)
    eng.dinov2_apply("rowscale", w=w, factor=f, prepared=out.view, rows=rows, cols=cols, dtype=dt)
    out.check("rowscale")
    prod = f.float().cpu().numpy()[:, None] * w.float().cpu().numpy()
    assert prod.dtype == np.float32
    want = torch.from_numpy(prod).to(BF16).view(I16).to(DEV)
    assert_bits(out.valid_bits(), want, f"rowscale dtype {dt}")
    wrong = torch.from_numpy(np.resize(f.float().cpu().numpy(), cols)[None, :] * w.float().cpu().numpy()).to(BF16).view(I16).to(DEV)
    assert_mutant_bits(wrong, want, rows * cols // 2, "the factor indexed by the column")
    ob = torch.full((rows + 8,), float("nan"), dtype=F32, device=DEV)
    eng.dinov2_apply("mul", w=b, factor=f, prepared=ob, rows=rows, dtype=dt)
    assert bool(torch.isnan(ob[rows:]).all())
    assert np.array_equal(ob[:rows].cpu().numpy().view(np.uint32), (f.float().cpu().numpy() * b.float().cpu().numpy()).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# (2) attention at 257 tokens


def _random_qkv(n, H, seed, q_scale=0.25):
    g = _gen(seed)
    x = torch.empty((n * T, 3, H * DH), dtype=BF16, device=DEV)
    x[:, 0] = _randn((n * T, H * DH), g, q_scale, BF16)
    x[:, 1] = _randn((n * T, H * DH), g, 1.0, BF16)
    x[:, 2] = _randn((n * T, H * DH), g, 1.0, BF16)
    return x.view(n * T, 3 * H * DH)


def _view(qkv, H):
    return qkv.view(-1, T, 3, H, DH)


def reference(qkv, H, mutant=None, crops=None):
    """float64 (out, A), each [n, T, H, dh]: s = q . k (Q carries dh^-0.5 log2 e), p = 2^(s - rowmax), out = sum p v / sum p,
    A = sum p |v| / sum p; mutant(s [n, H, T, T]) -> scores replaces the true scores (a named kernel bug); crops: those crops only"""
    x = _view(qkv, H)
    if crops is not None:
        x = x[torch.as_tensor(crops, device=DEV)]
    x = x.double()
    q, k, v = (x[:, :, j].permute(0, 2, 1, 3) for j in range(3))  # [n, H, T, dh]
    s = q @ k.transpose(-1, -2)
    if mutant:
        s = mutant(s)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p @ v) / l).permute(0, 2, 1, 3), ((p @ v.abs()) / l).permute(0, 2, 1, 3)


def _tol(ref, A):
    return 2.0**-8 * (ref.abs() + A)


def attend(eng, qkv, H, only_block=-1, out=None):
    n = qkv.shape[0] // T
    if out is None:
        buf = Guard(BF16, n * T, H * DH)
        eng.dinov2_apply("attention", qkv=qkv, out=buf.view, n=n, heads=H, only_block=only_block)
        buf.check("attn_mid")
        return buf.valid.clone()
    eng.dinov2_apply("attention", qkv=qkv, out=out, n=n, heads=H, only_block=only_block)
    return out


def check_close(got, ref, A, H, what):
    assert_close(got.view(-1, T, H, DH).double(), ref, _tol(ref, A), what)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_random(eng, H, n):
    qkv = _random_qkv(n, H, 100 + 7 * H + n)
    ref, A = reference(qkv, H)
    check_close(attend(eng, qkv, H), ref, A, H, f"attn_mid random H {H} n {n}")


def test_attention_crosses_the_persistent_stride(eng):
    """200 crops x 6 heads = 1200 items on a grid of 512 workgroups: every workgroup walks two or three items.  Every output is
    finite; the reference is taken on the crops that hold the first and the last item and the items around the grid's
    multiples (items 511..513 are crop 85, 1023..1025 crops 170 and 171)."""
    n, H = 200, 6
    qkv = _random_qkv(n, H, 5)
    got = attend(eng, qkv, H).view(n, T, H, DH)
    assert bool(torch.isfinite(got.float()).all())
    crops = [0, 84, 85, 86, 170, 171, 199]
    assert {511 // H, 512 // H, 513 // H, 1023 // H, 1024 // H, 1025 // H, (n * H - 1) // H} <= set(crops)
    ref, A = reference(qkv, H, crops=crops)
    check_close(got[torch.as_tensor(crops, device=DEV)].contiguous(), ref, A, H, "attn_mid n 200")


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_zero_queries_average_exactly_the_257_value_rows(eng, H):
    """Q = 0: every score is 0 and the output is the mean of the crop's own 257 V rows.  LDS rows 257..287 hold clamped copies
    of row 256: counted as keys they would weigh V[256] 32 times.  In the second launch the first 31 K and V rows of crop 1
    are huge (1e30): read unclamped and counted, they would drown crop 0's rows."""
    n = 2
    qkv = _random_qkv(n, H, 300 + H)
    x = _view(qkv, H)
    x[:, :, 0] = 0.0
    for huge in (False, True):
        if huge:
            x[1, :31, 1] = 1e30
            x[1, :31, 2] = 1e30
        ref, A = reference(qkv, H)
        mean = x[:, :, 2].double().mean(1, keepdim=True).expand(n, T, H, DH)
        assert bool(((ref - mean).abs() <= 1e-12 * A).all())  # the reference IS the mean
        got = attend(eng, qkv, H)
        check_close(got, ref, A, H, f"attn_mid Q = 0, H {H}, huge next crop {huge}")
        tol = _tol(ref, A)
        v = x[:, :, 2].double()
        counted = ((v.sum(1, keepdim=True) + 31 * v[:, 256:257]) / 288).expand(n, T, H, DH)  # the clamped copies as keys
        assert_mutant_far(counted[0], ref[0], tol[0], T * H * DH // 2, "padding rows counted as keys")
        if huge:
            spill = ((v[0].sum(0, keepdim=True) + v[1, :31].sum(0, keepdim=True)) / 288).expand(T, H, DH)  # crop 1's rows 0..30 as keys 257..287
            assert_mutant_far(spill, ref[0], tol[0], T * H * DH // 2, "unclamped reads into the next crop")


SPIKE_KEYS = (0, 31, 32, 255, 256)
SPIKE_ROWS = [0, 31, 32, 255, 256]


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_spikes_at_tile_and_padding_borders(eng, H):
    """Spike keys at the borders of the 32-key tiles and at key 256, the lone key of the last tile (whose clamped copies fill
    LDS rows 257..287), for queries at the borders of the query blocks and the lone query of the last one.  The planted
    queries are e0, so a planted row's scores are dim 0 of K exactly: 8 at the spike key, 0 at the 256 others -- the row's
    maximum sits at the spike (under spike 256: at key 256) and the spike holds half of the row's mass, so dropping it, and
    counting keys 257..259 (three more copies of key 256: four fifths of the mass), both move the output."""
    n = 3
    qkv = _random_qkv(n, H, 400 + H)
    x = _view(qkv, H)
    x[:, :, 1, :, 0] = 0.0  # dim 0 of K: zero except at the spike key
    key_of = torch.tensor([[SPIKE_KEYS[(i * H + h) % 5] for h in range(H)] for i in range(n)], device=DEV)
    for i in range(n):
        for h in range(H):
            x[i, int(key_of[i, h]), 1, h, 0] = 8.0
            x[i, SPIKE_ROWS, 0, h, :] = 0.0
            x[i, SPIKE_ROWS, 0, h, 0] = 1.0
    ref, A = reference(qkv, H)
    s = (x[:, :, 0].double().permute(0, 2, 1, 3) @ x[:, :, 1].double().permute(0, 2, 3, 1))[:, :, SPIKE_ROWS]  # [n, H, rows, T]
    at256 = key_of == 256
    assert bool(at256.any()) and bool((s.argmax(-1)[at256] == 256).all()), "no planted row has its maximum at key 256"
    check_close(attend(eng, qkv, H), ref, A, H, f"attn_mid spikes H {H}")
    tol = _tol(ref, A)
    onehot = torch.nn.functional.one_hot(key_of, T).bool()[:, :, None, :]  # [n, H, 1, T]

    def dropped(s):
        return s.masked_fill(onehot, float("-inf"))

    def key256_dropped(s):
        s = s.clone()
        s[..., 256] = float("-inf")
        return s

    def pad_counted(s):  # keys 257..259 are copies of key 256: key 256 weighs 4 x
        s = s.clone()
        s[..., 256] += 2.0
        return s

    for name, mutant in (("the spike key dropped", dropped), ("key 256 dropped", key256_dropped), ("keys 257..259 counted", pad_counted)):
        mref, _ = reference(qkv, H, mutant)
        ratio = ((mref - ref).abs() / tol)[:, SPIKE_ROWS].amax(-1)  # [n, rows, H]
        sel = ratio if mutant is dropped else ratio.permute(0, 2, 1)[at256]
        assert sel.numel() and bool((sel >= 4).all()), f"mutant '{name}' is not separated: {sel.min()}"


@pytest.mark.parametrize("H", [6, 12, 16])
def test_attention_huge_last_key(eng, H):
    """K row 256 is huge and finite (|k| = 1e30, scores of ~1e30 in either sign, finite in f32); its clamped copies in LDS rows
    257..287 carry the same scores and are removed by selection, never by adding a large negative number (which these scores
    would swallow): nothing but the 257 tokens reaches an output, and every output is finite."""
    n = 2
    qkv = _random_qkv(n, H, 500 + H)
    x = _view(qkv, H)
    x[:, 256, 1] = torch.where(x[:, 256, 1] > 0, 1e30, -1e30).to(BF16)
    ref, A = reference(qkv, H)
    assert bool(torch.isfinite(ref).all())
    got = attend(eng, qkv, H)
    assert bool(torch.isfinite(got.float()).all())
    check_close(got, ref, A, H, f"attn_mid huge key 256, H {H}")


@pytest.mark.parametrize("H", [6, 16])
def test_attention_only_block(eng, H):
    """only_block b computes and stores rows 32 b .. 32 b + 31 (block 8: row 256 alone) bit-identically to the full launch and
    leaves every other row of a sentinel-filled output as it is."""
    n = 3
    qkv = _random_qkv(n, H, 600 + H)
    full = attend(eng, qkv, H).view(I16).view(n, T, H * DH)
    for blk in range(9):
        rows = slice(32 * blk, min(32 * blk + 32, T))
        buf = Guard(BF16, n * T, H * DH)
        attend(eng, qkv, H, only_block=blk, out=buf.view)
        buf.check(f"only_block {blk}")
        got = buf.valid_bits().view(n, T, H * DH)
        assert_bits(got[:, rows].reshape(-1, H * DH), full[:, rows].reshape(-1, H * DH), f"only_block {blk}: the computed block")
        other = torch.ones(T, dtype=torch.bool, device=DEV)
        other[rows] = False
        assert bool((got[:, other] == SENT16).all()), f"only_block {blk}: the other blocks' rows were written"


def test_apply_refuses_bad_arguments(eng):
    qkv = _random_qkv(1, 6, 1)
    out = torch.empty((T, 384), dtype=BF16, device=DEV)
    for kw, msg in ((dict(heads=8), "heads == 6, 12 and 16"), (dict(heads=6, only_block=9), "only_block in -1..8"), (dict(heads=6, n=-1), "n = -1")):
        with pytest.raises(MmeError, match=msg):
            eng.dinov2_apply("attention", **{"qkv": qkv, "out": out, "n": 1, **kw})
    with pytest.raises(MmeError, match="op 6 outside 0..5"):
        eng.dinov2_apply(6)
    with pytest.raises(MmeError, match="src != dst"):
        eng.dinov2_apply("retile", src=out, dst=out, n=1)
    with pytest.raises(MmeError, match="d == 384, d == 768 and d == 1024"):
        eng.dinov2_apply("embed_rows", d=512, n=1)
    with pytest.raises(MmeError, match="cols a multiple of 8"):
        eng.dinov2_apply("rowscale", w=out, factor=out, prepared=out, rows=4, cols=12, dtype=1)


# ---------------------------------------------------------------------------------------------------------------------
# (3) prepared buffers


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_prepared_buffers_host_and_device(tmp_path, dtype):
    """A directory with the 1370-row table, in each element type: the device preparer (the file's own bytes) and the host
    preparer (the same values widened to f32) leave equal fingerprints and equal bytes; o_w / o_b / fc2_w / fc2_b hold the
    float64 product with LayerScale rounded ONCE (the seeded values have at most 11 significant bits, so the f32 product the
    preparers form is exact); pos is the interpolated f32 table; patch_w is [D, 640] with zero columns behind 588."""
    geom = dataclasses.replace(DINOV2_B14, hidden_size=384, num_heads=6, num_layers=2, intermediate_size=128)
    ckpt.save_checkpoint(tmp_path, make_dinov2_weights(21, geom, pos_grid=37), "dinov2", dtype, geometry=geom)
    ck = ckpt.read_checkpoint(tmp_path, "dinov2")
    assert ck.dtype == dtype and ck.geometry == dataclasses.replace(geom, position_grid=37)
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_dinov2_checkpoint(ck)
        host.load_dinov2({k: t.float().numpy() for k, t in ck.tensors.items()})
        fd, fh = dev.weights_fingerprint(), host.weights_fingerprint()
        bd = [dev.weights_read(i) for i in range(len(fd))]
        bh = [host.weights_read(i) for i in range(len(fh))]
        info, g = dev.encoder_info(), dev.vit_geometry()
    finally:
        dev.close()
        host.close()
    D, F, L = geom.hidden_size, geom.intermediate_size, geom.num_layers
    assert info == {"kind": "dinov2", "embed_dim": D, "hidden_act": "gelu", "projection_dim": None}
    assert (g.patch_size, g.seq_len, g.hidden_size, g.num_layers) == (14, T, D, L)
    assert len(bd) == len(bh) == 6 + 18 * L and fd == fh
    for i, (a, b) in enumerate(zip(bd, bh)):
        assert a.size == b.size and np.array_equal(a, b), f"buffer [{i}] differs between the device and the host preparer"
    m = {k: t.double().numpy() for k, t in ck.tensors.items()}
    assert np.array_equal(bd[1].view(np.float32).reshape(T, D), ck.extra["position_table"].numpy())
    pw = bd[5].view(np.uint16).reshape(D, KP)
    assert not pw[:, 588:].any()
    assert np.array_equal(pw[:, :588], round_to_bf16(m["embeddings.patch_embeddings.projection.weight"].reshape(D, 588).astype(np.float32)).view(np.uint32) >> 16)

    def bf16_once(x64):
        x32 = x64.astype(np.float32)
        assert np.array_equal(x32.astype(np.float64), x64), "the product is not exact in float32"
        return (round_to_bf16(x32).view(np.uint32) >> 16).astype(np.uint16)

    for l in range(L):
        p, base = f"encoder.layer.{l}.", 6 + 18 * l
        l1, l2 = m[p + "layer_scale1.lambda1"], m[p + "layer_scale2.lambda1"]
        assert l1.std() > 0.2 and l2.std() > 0.2
        want = {9: bf16_once(l1[:, None] * m[p + "attention.output.dense.weight"]), 16: bf16_once(l2[:, None] * m[p + "mlp.fc2.weight"])}
        for i, w in want.items():
            got = bd[base + i].view(np.uint16).reshape(w.shape)
            assert np.array_equal(got, w), f"layer {l} buffer {i}"
            unscaled = bf16_once(m[p + ("attention.output.dense.weight" if i == 9 else "mlp.fc2.weight")])
            assert (unscaled != w).sum() > w.size // 2, "LayerScale left out would not be caught"
            by_col = bf16_once((l1 if i == 9 else l2)[None, :] * m[p + "attention.output.dense.weight"]) if i == 9 else None
            assert by_col is None or (by_col != w).sum() > w.size // 2, "lambda applied to the input columns would not be caught"
        for i, lam, name in ((10, l1, "attention.output.dense.bias"), (17, l2, "mlp.fc2.bias")):
            prod = lam * m[p + name]
            assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)
            assert np.array_equal(bd[base + i].view(np.float32), prod.astype(np.float32)), f"layer {l} buffer {i}"


# ---------------------------------------------------------------------------------------------------------------------
# (4) end to end


@pytest.mark.parametrize("key, pool", [("S14", "cls"), ("B14", "cls"), ("L14", "cls"), ("B14", "last")])
def test_end_to_end_against_the_restatement_and_transformers(golden_dir, key, pool):
    from oracle import preprocess as opre

    seed, geom, grid = CASES[key]
    w = weights_of(key)
    arrays = list(synthetic_crops(mkd.N_CROPS, seed=0)) + _golden_crops(golden_dir)
    assert len(arrays) == 40
    pv = np.stack([opre.preprocess_crop(a) for a in arrays]).astype(np.float32)
    emb = RegionEmbedder(device=0, encoder="dinov2", weights=w, geometry=geom, pool=pool, chunk=64)
    try:
        assert emb.embed_dim == geom.hidden_size and emb.engine.vit_geometry().patch_size == 14 and emb.pool_token == (0 if pool == "cls" else 256)
        pix, offs, hw = _pack(arrays)
        e32, e16 = emb.embed_packed(pix, offs, hw)
        torch.cuda.synchronize()
        assert emb.engine.attention_redone(geom.num_layers) == [0] * geom.num_layers
        got = e32.cpu().numpy()
        assert got.shape == (40, geom.hidden_size) and np.array_equal(e16.float().cpu().numpy(), round_to_bf16(got))
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)
        assert rows.shape == (3, geom.hidden_size) and ok.all() and np.array_equal(rows, got[:3])
        with pytest.raises(NotImplementedError):
            emb.get_text_embeddings(["a query"])
    finally:
        _close_all(emb)
    want = dr.dinov2_embed(pv, w, geom, torch.float32, token=0 if pool == "cls" else 256)
    omc = dr.one_minus_cos(got, want)
    print(f"dinov2 parity {key} pool {pool} ({geom.hidden_size}-d x {geom.num_layers} layers): max(1 - cos) = {omc.max():.3g} "
          f"(synthetic 224^2: {omc[:16].max():.3g}, bundled: {omc[16:].max():.3g})")
    assert float(omc.max()) <= 1e-3, (key, float(omc.max()))
    mu = want.mean(axis=0, keepdims=True)
    a, b = got - mu, want - mu  # centred: near-identical seeded-weight embeddings cannot pass trivially
    ccos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert np.all(ccos > 0.98), (key, float(ccos.min()))
    if pool == "cls":
        rec = np.load(os.path.join(golden_dir, "dinov2_cases.npz"))[f"{key}.pooler_output"]
        omc_hf = dr.one_minus_cos(got[:16], rec)
        print(f"dinov2 parity {key}: against the recorded transformers rows max(1 - cos) = {omc_hf.max():.3g}")
        assert float(omc_hf.max()) <= 1e-3, (key, float(omc_hf.max()))


def test_checkpoint_directory_with_the_1370_row_table(tmp_path, crops40):
    """RegionEmbedder(dir, encoder="dinov2") on a saved bf16 directory whose position table is 37 x 37 equals the embedder on
    the same weight dict bit for bit (under the directory's image_mean / image_std), and has no text tower."""
    key = "S14p37"
    seed, geom, grid = CASES[key]
    w = weights_of(key)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ckpt.save_checkpoint(tmp_path, w, "dinov2", "bfloat16", geometry=geom, image_mean=mean, image_std=std)
    by_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="dinov2")
    by_dict = RegionEmbedder(device=0, chunk=64, encoder="dinov2", weights=w)
    try:
        ck = by_dir.checkpoint
        assert ck.dtype == "bfloat16" and ck.geometry.position_grid == 37 and tuple(ck.tensors[POS].shape) == (1, 1370, 384)
        assert by_dir.engine.weights_fingerprint() == by_dict.engine.weights_fingerprint()
        a32, a16 = by_dict.embed_uniform(crops40)
        torch.cuda.synchronize()
        by_dict.engine.set_normalisation(mean, std)
        b32, b16 = by_dict.embed_uniform(crops40)
        c32, c16 = by_dir.embed_uniform(crops40)
        torch.cuda.synchronize()
        assert torch.equal(b32, c32) and torch.equal(b16, c16) and bool(torch.isfinite(c32).all()) and tuple(c32.shape) == (40, 384)
        assert not torch.equal(a32, b32)  # the directory's image_mean / image_std were applied
        with pytest.raises(NotImplementedError, match="no text tower"):
            by_dir.get_text_embeddings(["a query"])
    finally:
        _close_all(by_dir)
        _close_all(by_dict)


def test_the_interpolated_table_against_transformers(golden_dir):
    """The S14 tower with a 37 x 37 position table against what Dinov2Model returned under image_size 518.  (The seeded position
    rows are small beside the patch embedding, so this bound alone would not tell an uninterpolated table apart: that the
    device holds the model's own interpolated table bit for bit is test_prepared_buffers_host_and_device's and
    tests/test_dinov2_cpu.py's.)"""
    key = "S14p37"
    seed, geom, grid = CASES[key]
    w = weights_of(key)
    eng = Engine(0)
    try:
        eng.load_dinov2(w)
        eng.set_chunk(64)
        got = _uniform(eng, torch.from_numpy(synthetic_crops(mkd.N_CROPS, seed=0)).cuda())[0].cpu().numpy()
    finally:
        eng.close()
    rec = np.load(os.path.join(golden_dir, "dinov2_cases.npz"))[f"{key}.pooler_output"]
    omc = dr.one_minus_cos(got, rec)
    print(f"dinov2 parity {key} (position table 37 x 37 -> 16 x 16): against the recorded transformers rows max(1 - cos) = {omc.max():.3g}")
    assert float(omc.max()) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# (5) bit identities


@pytest.mark.parametrize("key", ["S14", "L14"])
def test_forward_settings_are_bit_identical(crops40, key):
    """ln_mode 1 = 2, every GEMM variant, pruned = unpruned at tokens in four query blocks, chunking (5 crops in chunks of 2
    among them), tile order, attention mode.  72 crops = 18 504 rows: interior 256-row tiles and a ragged one."""
    seed, geom, grid = CASES[key]
    eng = Engine(0)
    try:
        eng.load_dinov2(weights_of(key), geom)
        crops = torch.cat([crops40, torch.from_numpy(synthetic_crops(32, seed=9)).cuda()])
        eng.set_chunk(72)
        eng.set_ln_fusion(1)
        ref, _ = _uniform(eng, crops)
        assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (72, geom.hidden_size)
        for variant in (0, 1, 3, 4, 6):
            eng.set_gemm_variant(variant)
            for mode in (2, 1):
                eng.set_ln_fusion(mode)
                got, _ = _uniform(eng, crops)
                assert torch.equal(ref, got), (key, "gemm variant", variant, "ln fusion", mode)
        eng.set_gemm_variant(0)
        eng.set_ln_fusion(2)
        for tok in (0, 31, 32, 255, 256):
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
        assert torch.equal(c64, ref[:40]), (key, "the same crops inside a pass of 72")
        eng.set_chunk(2)
        c2, _ = _uniform(eng, crops40[:5])
        assert torch.equal(c2, c64[:5]), (key, "5 crops in chunks of 2")
        # mme_embed = mme_preprocess, then mme_vit_forward (the caller's [n * 256, 640] matrix, chunked)
        per = 224 * 224 * 3
        patches = eng.preprocess(crops40[:5].reshape(-1), np.arange(5, dtype=np.int64) * per, np.full((5, 2), 224, np.int32))
        assert tuple(patches.shape) == (5 * NP, KP)
        sep, _ = eng.vit_forward(patches)
        torch.cuda.synchronize()
        assert torch.equal(sep, c2), (key, "preprocess + forward")
        eng.set_chunk(8)
        for order in (0, 2, 1):
            eng.set_tile_order(order)
            got, _ = _uniform(eng, crops40)
            assert torch.equal(got, c8), (key, "tile order", order)
        for mode in (0, 2, 1):  # the attention mode keeps its value and changes nothing at 257 tokens
            eng.set_attention_mode(mode)
            got, _ = _uniform(eng, crops40)
            assert torch.equal(got, c8) and eng.attention_redone(geom.num_layers) == [0] * geom.num_layers, (key, "attention mode", mode)
        with pytest.raises(MmeError, match="mme_dinov2_apply op 2 launches its kernel"):
            eng.attention(torch.zeros((197, 3 * geom.hidden_size), dtype=BF16, device=DEV), 0)
        with pytest.raises(MmeError, match="pool_token 257 outside 0..256"):
            _uniform(eng, crops40[:1], 257)
    finally:
        eng.close()


def test_layernorm_kernel_mode_against_the_restatement():
    from oracle import preprocess as opre

    seed, geom, grid = CASES["S14"]
    w = weights_of("S14")
    crops = synthetic_crops(16, seed=0)
    pv = np.stack([opre.preprocess_crop(a) for a in crops]).astype(np.float32)
    eng = Engine(0)
    try:
        eng.load_dinov2(w, geom)
        eng.set_chunk(64)
        eng.set_ln_fusion(0)
        got0 = _uniform(eng, torch.from_numpy(crops).cuda())[0].cpu().numpy()
    finally:
        eng.close()
    omc0 = dr.one_minus_cos(got0, dr.dinov2_embed(pv, w, geom, torch.float32))
    print(f"dinov2 parity S14, LayerNorm-kernel mode: max(1 - cos) = {omc0.max():.3g}")
    assert float(omc0.max()) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# (6) coexistence on one context


def test_clip16_then_dinov2_then_clip16_on_one_context(crops40):
    g16 = dataclasses.replace(CLIP_B16, num_layers=2)
    w16 = make_clip_weights(15, g16)
    seed, g14, grid = CASES["B14"]
    w14 = weights_of("B14")
    fresh = Engine(0)
    try:
        fresh.load_dinov2(w14, g14)
        fresh.set_chunk(64)
        solo14 = [t.clone() for t in _uniform(fresh, crops40)]
    finally:
        fresh.close()
    e = Engine(0)
    try:
        e.set_chunk(64)
        e.load_clip(w16, g16)
        first = [t.clone() for t in _uniform(e, crops40)]
        fp16 = e.weights_fingerprint()
        assert e.encoder_info()["kind"] == "clip" and e.vit_geometry().patch_size == 16
        e.load_dinov2(w14, g14)
        assert e.encoder_info()["kind"] == "dinov2" and e.vit_geometry().patch_size == 14 and e.vit_geometry().seq_len == T
        second = _uniform(e, crops40)
        assert torch.equal(second[0], solo14[0]) and torch.equal(second[1], solo14[1])
        e.load_clip(w16, g16)
        assert e.encoder_info()["kind"] == "clip" and e.vit_geometry().patch_size == 16 and e.weights_fingerprint() == fp16
        third = _uniform(e, crops40)
        assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])
        assert first[0].shape != second[0].shape or not torch.equal(first[0], second[0])
        # the other loaders keep refusing patch 14, and what the context held stays
        with pytest.raises(MmeError, match=r"mme_load_clip: patch_size = 14; supported: 16, 32"):
            e.load_clip(make_clip_weights(15, dataclasses.replace(g16, patch_size=14)), dataclasses.replace(g16, patch_size=14))
        again = _uniform(e, crops40)
        assert torch.equal(again[0], first[0])
    finally:
        e.close()
