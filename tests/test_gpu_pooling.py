"""Mean pooling over the patches a crop covers (pool = "mean", "cls+mean") on the GPU.

1. The single launch (mme_pool_apply) against float64, element by element, on the planted blocks of tests/pooling_reference.py:
   d 384 / 768 / 1024 x (tokens, g) = (197, 14), (50, 7), (257, 16) x both ops, twelve blocks with the nine grids (g, g), (1, 1),
   (1, g), (g, 1), (5, g), (g, 5), (g - 1, g - 1), (2, 3), (10, 14) (capped at g) and a block with a row shifted by + 30, one
   with a row scaled x 100 and a zero block.  The rule of tests/test_gpu_gemm.py (e): the bf16 output is the RNE of the f32
   output bit for bit; the f32 output sits within 8 x the largest deviation of a float32 numpy restatement from the float64 one
   on the same inputs, never below 2^-22; guard rows stay; every mutant of the reference leaves 4 x that tolerance on at least
   B * d / 2 elements (tests/test_pooling_cpu.py measures them: 1e-4 and more against a tolerance of 2.4e-7).  The grid (1, 1) is
   rowop_apply("pool_ln_l2", tok = 1) bit for bit.  Refusals by message, outputs untouched.
2. Whole towers (hidden 384, MLP 64, one layer, six heads, seeded: SMALL of tests/test_gpu_tokens.py; ViT/16, ViT/32, DINOv2) on
   crops of 224 x 224, 90 x 300, 333 x 120, 4 x 400, 160 x 224 and 161 x 224 through chunks of two, pruning on and off:
   (a) both modes against the float64 reference on the pixels Engine.preprocess produced, max(1 - cos) <= 1e-3, after (f) the
       required mutants were found more than 4e-3 from the reference on at least one crop;
   (b) mme_embed = mme_preprocess + mme_vit_forward_grids(mme_pool_grids) bit for bit: chunk 2 against one chunk, pruning on
       against off, f32 and bf16, a second identical call;
   (c) mme_vit_forward under a mean mode = mme_vit_forward_grids(NULL); mme_embed_tokens' pooled outputs = mme_embed's and its
       token rows those of mode 0;
   (d) under a resize spec the grids are whole;
   (e) a mode-0 forward after a mode-1 call is the one before it, the pruning setting stays, a load resets the mode: every
       image-tower load, the tile tower's beside a ViT tower that stays usable included; a text-tower load does not;
   (g) refusals by message; (h) RegionEmbedder; (i) mme_vit_forward_grids on a side stream (tests/stream_probes.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pooling_reference as pr  # noqa: E402
from test_gpu_gemm import BF16, DEV, F32, Guard, assert_bits  # noqa: E402
from test_gpu_tokens import SMALL, TOWERS  # noqa: E402

from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.staging import packed_layout  # noqa: E402

pytestmark = pytest.mark.gpu

I16, I32 = torch.int16, torch.int32
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
    e = Engine(0)  # a bare context: the single launch needs no tower
    yield e
    e.close()


def bits(t):
    return t.contiguous().view(I16 if t.dtype == BF16 else I32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the single launch


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def launch(eng, op, X, gm, bt, G, B, tokens, g, d, want=("f32", "bf16")):
    E = d * (2 if op == "cls+mean" else 1)
    e32, e16 = Guard(F32, B, E), Guard(BF16, B, E)
    eng.pool_apply(op, x=X, gamma=gm, beta=bt, grids=G, B=B, tokens=tokens, g=g, first=1, d=d, eps=pr.EPS,
                   emb_f32=e32.view if "f32" in want else None, emb_bf16=e16.view if "bf16" in want else None)
    e32.check(f"{op} f32")
    e16.check(f"{op} bf16")
    return e32, e16


@pytest.mark.parametrize("op", ["mean", "cls+mean"])
@pytest.mark.parametrize("tokens, g", pr.SHAPES)
@pytest.mark.parametrize("d", pr.WIDTHS)
def test_single_launch_against_float64(eng, d, tokens, g, op):
    x, gamma, beta, grids = pr.planted(d, tokens, g)
    B = len(grids)
    X, gm, bt, G = dev(x.reshape(B * tokens, d), BF16), dev(gamma), dev(beta), dev(grids)
    assert torch.equal(X.float().cpu(), torch.from_numpy(x.reshape(B * tokens, d))), "the planted values are bf16 values"
    e32, e16 = launch(eng, op, X, gm, bt, G, B, tokens, g, d)
    got = e32.valid.clone()
    assert bool(torch.isfinite(got).all())
    assert_bits(e16.valid_bits(), got.to(BF16).view(I16), f"{op}: bf16 output vs RNE of the f32 output")
    ref = pr.planted_reference(x, gamma, beta, grids, op, np.float64)
    yard = float(np.abs(pr.planted_reference(x, gamma, beta, grids, op, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    err = np.abs(got.double().cpu().numpy() - ref)
    print(f"pool_apply {op} d {d} tokens {tokens}: float32 yardstick {yard:.3g}, kernel max deviation {err.max():.3g}, tolerance {tol:.3g}")
    assert err.max() <= tol, f"{op} d {d} tokens {tokens}: max deviation {err.max():.3g} > {tol:.3g} at {np.unravel_index(err.argmax(), err.shape)}"
    bn = beta.astype(np.float64) / np.linalg.norm(beta.astype(np.float64))
    zero = got[11].double().cpu().numpy()
    zero = zero / np.linalg.norm(zero[-d:])  # cls+mean: both halves are beta; the mean half rescaled to a unit vector
    assert float(np.abs(zero[-d:] - bn).max()) <= 4 * tol, "zero block: the mean is not beta / ||beta||"
    # every mutant of the definition is far outside what the comparison above admits
    mutants = [m for m in pr.MUTANTS if op == "cls+mean" or m not in ("divide_by_g2", "l2_per_half")]
    for m in mutants:
        n = int((np.abs(pr.planted_reference(x, gamma, beta, grids, op, np.float64, m) - ref) > 4 * tol).sum())
        assert n >= B * d // 2, f"mutant '{m}' leaves 4 x the tolerance on {n} elements only (< {B * d // 2}): the case would not catch it"
    # one output requested: the same bits; NULL grids: whole grids
    only16 = launch(eng, op, X, gm, bt, G, B, tokens, g, d, want=("bf16",))
    assert only16[0].untouched() and torch.equal(only16[1].valid_bits(), e16.valid_bits())
    only32 = launch(eng, op, X, gm, bt, G, B, tokens, g, d, want=("f32",))
    assert only32[1].untouched() and torch.equal(only32[0].valid_bits(), e32.valid_bits())
    whole = launch(eng, op, X, gm, bt, dev(np.full((B, 2), g, np.int32)), B, tokens, g, d)
    null = launch(eng, op, X, gm, bt, None, B, tokens, g, d)
    assert_bits(null[0].valid_bits(), whole[0].valid_bits(), f"{op}: NULL grids against (g, g)")
    assert_bits(whole[0].valid_bits()[0], e32.valid_bits()[0], f"{op}: block 0, whose grid is (g, g)")


@pytest.mark.parametrize("d", pr.WIDTHS)
def test_grid_one_by_one_is_k8_bit_for_bit(eng, d):
    """(1, 1) covers token 1 alone: the accumulators start from the first row and 1.0f / 1 is exact"""
    tokens, g = 197, 14
    x, gamma, beta, grids = pr.planted(d, tokens, g)
    B = len(grids)
    X, gm, bt = dev(x.reshape(B * tokens, d), BF16), dev(gamma), dev(beta)
    e32, e16 = launch(eng, "mean", X, gm, bt, dev(np.ones((B, 2), np.int32)), B, tokens, g, d)
    k32, k16 = Guard(F32, B, d), Guard(BF16, B, d)
    eng.rowop_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, B=B, tok=1, d=d, eps=pr.EPS, emb_f32=k32.view, emb_bf16=k16.view)
    assert_bits(e32.valid_bits(), k32.valid_bits(), f"d {d}: f32 against pool_ln_l2(tok = 1)")
    assert_bits(e16.valid_bits(), k16.valid_bits(), f"d {d}: bf16 against pool_ln_l2(tok = 1)")
    # and the class half of cls+mean carries K8's direction for tok = 0
    c32, _ = launch(eng, "cls+mean", X, gm, bt, dev(np.ones((B, 2), np.int32)), B, tokens, g, d)
    eng.rowop_apply("pool_ln_l2", x=X, gamma=gm, beta=bt, B=B, tok=0, d=d, eps=pr.EPS, emb_f32=k32.view, emb_bf16=k16.view)
    half = c32.valid[:, :d].double()
    assert float((half / half.norm(dim=1, keepdim=True) - k32.valid.double()).abs().max()) <= 2.0**-22


def test_pool_apply_refuses_bad_arguments(eng):
    d, tokens, g = 384, 50, 7
    x, gamma, beta, grids = pr.planted(d, tokens, g)
    B = len(grids)
    X, gm, bt, G = dev(x.reshape(B * tokens, d), BF16), dev(gamma), dev(beta), dev(grids)
    e32, e16 = Guard(F32, B, 2 * d), Guard(BF16, B, 2 * d)
    base = dict(x=X, gamma=gm, beta=bt, grids=G, B=B, tokens=tokens, g=g, first=1, d=d, eps=pr.EPS, emb_f32=e32.view, emb_bf16=e16.view)
    shifted = torch.zeros(B * tokens * d + 8, dtype=BF16, device=DEV)[1:]
    bad_g = grids.copy()
    cases = [(dict(x=None), "op 0 needs x, gamma, beta non-null and 16-byte aligned"), (dict(gamma=None), "x, gamma, beta non-null"),
             (dict(x=shifted), "x, gamma, beta non-null and 16-byte aligned"), (dict(beta=bt[1:]), "16-byte aligned"),
             (dict(emb_f32=None, emb_bf16=None), "op 0 needs emb_f32 or emb_bf16"), (dict(emb_f32=e32.view.view(-1)[1:]), "emb_f32 and emb_bf16 16-byte aligned"),
             (dict(grids=G.view(-1)[1:]), "grids 8-byte aligned"), (dict(d=1280), r"op 0 is built for d == 384, d == 768 and d == 1024 \(d = 1280\)"),
             (dict(B=-1), "B = -1 outside"), (dict(g=17, tokens=290), "g = 17; supported 1..16"), (dict(first=2), "first = 2; supported 0 and 1"),
             (dict(tokens=49), r"tokens = 49; supported first \+ g \* g = 50")]
    for over, text in cases:
        with pytest.raises(MmeError, match="mme_pool_apply: " + ".*" + text if not text.startswith("op") else "mme_pool_apply: " + text):
            eng.pool_apply(0, **{**base, **over})
    with pytest.raises(MmeError, match=r"mme_pool_apply: op 1 \(cls\+mean\) needs first == 1"):
        eng.pool_apply(1, **{**base, "first": 0, "tokens": 49})
    with pytest.raises(MmeError, match="mme_pool_apply: op 2 outside 0..1"):
        eng.pool_apply(2, **base)
    # the device grids are checked by the caller-side wrapper, entry by entry
    for value, where in ((0, (3, 1)), (g + 1, (8, 0))):
        bad_g[:] = grids
        bad_g[where] = value
        with pytest.raises(MmeError, match=rf"pool_apply: grids\[{where[0]}\]\[{where[1]}\] = {value}; supported 1\.\.{g}"):
            eng.pool_apply(0, **{**base, "grids": dev(bad_g)})
    torch.cuda.synchronize()
    assert e32.untouched() and e16.untouched(), "a refused call wrote to its outputs"


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole towers

SIZES = [(224, 224), (90, 300), (333, 120), (4, 400), (160, 224), (161, 224)]
GRIDS16 = [(14, 14), (5, 14), (14, 5), (1, 14), (10, 14), (11, 14)]
N, D = len(SIZES), 384
KEYS = ["vit16", "vit32", "dinov2"]
MODES = ["mean", "cls+mean"]
REQUIRED = {"mean": ("whole_grid", "grid_transposed", "row_short"), "cls+mean": ("whole_grid", "grid_transposed", "row_short", "divide_by_g2")}
# cls_in_mean is required where the reference holds it apart: at patch 32 one more row among at most 49 moves the mean by
# 5.8e-3 .. 1.0e-2; at patch 16 and 14 (up to 196 and 256 rows) it stays at 1.0e-3 .. 2.5e-3 and is recorded
REQUIRED_BY_TOWER = {"vit32": ("cls_in_mean",)}


@pytest.fixture(scope="module")
def crops():
    rng = np.random.default_rng(11)
    arrays = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    hw = np.array(SIZES, dtype=np.int32)
    offs, sizes, total = packed_layout(hw)
    buf = np.zeros(total, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(DEV), offs, hw


def tower(key, seed=7, chunk=2):
    loader, geom, make, T, _ = TOWERS[key]
    e = Engine(0)
    getattr(e, loader)(make(seed, geom), geom=geom)
    e.set_chunk(chunk)
    return e, geom, make(seed, geom)


def pixels_of(patches, n, patch):
    """the bf16 patch matrix of Engine.preprocess (rows (crop, gy, gx), columns (c, ky, kx), zero columns behind at patch 14)
    -> float64 pixel values [n, 3, 224, 224]"""
    g = 224 // patch
    x = patches[:, : 3 * patch * patch].double().cpu().view(n, g, g, 3, patch, patch)
    return x.permute(0, 3, 1, 4, 2, 5).reshape(n, 3, 224, 224).numpy()


_reference = {}


def reference(key, crops):
    """(grids, y float64 [N, T, D]: the final-LayerNorm rows of the float64 tower on the engine's own pixels), once per tower"""
    if key not in _reference:
        e, geom, w = tower(key)
        try:
            patches = e.preprocess(*crops)
            grids = e.pool_grids(crops[2])
            torch.cuda.synchronize()
        finally:
            e.close()
        kind = "dinov2" if key == "dinov2" else "vit"
        _reference[key] = (grids, pr.final_ln_rows(kind, pixels_of(patches, N, geom.patch_size), w, geom, torch.float64))
    return _reference[key]


def ref_vectors(key, crops, mode, mutant=None):
    grids, y = reference(key, crops)
    return np.stack([pr.pooled(y[b], grids[b], mode, mutant) for b in range(N)])


@pytest.mark.parametrize("key", KEYS)
def test_towers_against_the_float64_reference(crops, key):
    grids, y = reference(key, crops)
    patch = TOWERS[key][1].patch_size
    assert [tuple(r) for r in grids.tolist()] == [pr.covered_grid(h, w, patch) for h, w in SIZES]
    if patch == 16:
        assert [tuple(r) for r in grids.tolist()] == GRIDS16
    # (f) sharpness, on the float64 reference before the engine is asked: each required mutant is more than 4 x the bound away on a crop
    for mode in MODES:
        ref = ref_vectors(key, crops, mode)
        for m in pr.MUTANTS:
            if mode == "mean" and m in ("divide_by_g2", "l2_per_half"):
                continue
            far = pr.one_minus_cos(ref_vectors(key, crops, mode, m), ref)
            required = m in REQUIRED[mode] + REQUIRED_BY_TOWER.get(key, ())
            # cls_in_mean and the others outside REQUIRED are held at the tower level only where this figure says so (one
            # row in P + 1 moves a mean little at patch 16 and 14); the single-launch test holds every mutant in every case
            status = "required" if required else ("recorded: beyond 4e-3, held here too" if far.max() > 4e-3 else "recorded: within 4e-3, held by the single launch only")
            print(f"{key} {mode} mutant {m}: max(1 - cos) over the crops = {far.max():.3g} at crop {int(far.argmax())} ({status})")
            if required:
                assert far.max() > 4e-3, (key, mode, m, far.tolist())
    e, geom, _ = tower(key)
    try:
        for mode in MODES:
            e.set_pooling(mode)
            assert e.pooling == mode and e.embed_dim == (2 * D if mode == "cls+mean" else D)
            ref = ref_vectors(key, crops, mode)
            for prune in (False, True):
                e.set_forward_pruning(prune)
                e32, e16 = e.embed(*crops)
                torch.cuda.synchronize()
                assert tuple(e32.shape) == tuple(e16.shape) == ref.shape
                assert_bits(bits(e16), bits(e32.to(BF16)), f"{key} {mode}: bf16 output vs RNE of the f32 output")
                got = e32.double().cpu().numpy()
                assert float(np.abs(np.linalg.norm(got, axis=1) - 1.0).max()) <= 1e-5
                err = pr.one_minus_cos(got, ref)
                print(f"{key} {mode} prune {prune}: 1 - cos per crop = {[f'{v:.2g}' for v in err]}")
                assert err.max() <= 1e-3, (key, mode, prune, err.tolist())
    finally:
        e.close()


@pytest.mark.parametrize("key", KEYS)
def test_embed_is_preprocess_then_forward_with_the_grids(crops, key):
    e, geom, _ = tower(key)
    try:
        patches = e.preprocess(*crops)
        grids = e.pool_grids(crops[2])
        seen = {}
        for mode in MODES:
            e.set_pooling(mode)
            for chunk in (2, 8):
                for prune in (False, True):
                    e.set_chunk(chunk)
                    e.set_forward_pruning(prune)
                    a32, a16 = e.embed(*crops)
                    b32, b16 = e.vit_forward(patches, grids=grids)
                    c32, c16 = e.embed(*crops)
                    torch.cuda.synchronize()
                    what = f"{key} {mode} chunk {chunk} prune {prune}"
                    assert_bits(bits(a32), bits(b32), what + ": embed against preprocess + vit_forward_grids, f32")
                    assert_bits(bits(a16), bits(b16), what + ": bf16")
                    assert_bits(bits(c32), bits(a32), what + ": a second identical call")
                    first = seen.setdefault(mode, (a32, a16))
                    assert_bits(bits(a32), bits(first[0]), what + ": against chunk 2 without pruning, f32")
                    assert_bits(bits(a16), bits(first[1]), what + ": bf16")
            # one output at a time
            only32, none16 = e.embed(*crops, want_bf16=False)
            none32, only16 = e.embed(*crops, want_f32=False)
            assert none16 is None and none32 is None
            assert_bits(bits(only32), bits(seen[mode][0]), f"{key} {mode}: f32 alone")
            assert_bits(bits(only16), bits(seen[mode][1]), f"{key} {mode}: bf16 alone")
        # the two modes agree on the mean's direction, and the covered mean is not the whole one
        m, cm = seen["mean"][0].double(), seen["cls+mean"][0].double()[:, D:]
        assert float((m - cm / cm.norm(dim=1, keepdim=True)).abs().max()) <= 1e-6
        e.set_pooling("mean")
        w32, _ = e.vit_forward(patches)
        torch.cuda.synchronize()
        assert_bits(bits(w32[0]), bits(seen["mean"][0][0]), f"{key}: the 224 x 224 crop covers the whole grid")
        assert float((1 - (w32.double() * m).sum(1))[1:].min()) > 4e-3, "whole grids on ragged crops are other vectors"
    finally:
        e.close()


@pytest.mark.parametrize("key", KEYS)
def test_whole_grid_entry_points_and_token_rows(crops, key):
    e, geom, _ = tower(key)
    T = TOWERS[key][3]
    try:
        patches = e.preprocess(*crops)
        tok0, _, _ = e.embed_tokens(*crops)
        for mode in MODES:
            e.set_pooling(mode)
            E = e.embed_dim
            w32, w16 = e.vit_forward(patches, pool_token=T - 1)  # the token is checked and not used
            n32 = torch.zeros((N, E), dtype=F32, device=DEV)
            e._check(e.lib.mme_vit_forward_grids(e.h, patches.data_ptr(), N, None, n32.data_ptr(), None, e._stream()), "mme_vit_forward_grids")
            g = 224 // geom.patch_size
            f32, _ = e.vit_forward(patches, grids=np.full((N, 2), g, np.int32))
            t_tok, t32, t16 = e.vit_tokens(patches)
            torch.cuda.synchronize()
            assert_bits(bits(w32), bits(n32), f"{key} {mode}: mme_vit_forward against mme_vit_forward_grids(NULL)")
            assert_bits(bits(w32), bits(f32), f"{key} {mode}: against explicit whole grids")
            assert_bits(bits(t32), bits(w32), f"{key} {mode}: mme_vit_tokens pools whole grids, f32")
            assert_bits(bits(t16), bits(w16), f"{key} {mode}: bf16")
            a32, a16 = e.embed(*crops)
            tok, p32, p16 = e.embed_tokens(*crops)
            torch.cuda.synchronize()
            assert_bits(bits(p32), bits(a32), f"{key} {mode}: the pooled outputs of mme_embed_tokens against mme_embed, f32")
            assert_bits(bits(p16), bits(a16), f"{key} {mode}: bf16")
            assert_bits(bits(tok).view(N, -1), bits(tok0).view(N, -1), f"{key} {mode}: the token rows are those of mode 0")
            assert_bits(bits(t_tok).view(N, -1), bits(tok0).view(N, -1), f"{key} {mode}: mme_vit_tokens' rows")
            with pytest.raises(MmeError, match=rf"mme_vit_forward: pool_token {T} outside 0..{T - 1}"):
                e.vit_forward(patches, pool_token=T)
    finally:
        e.close()


def test_under_a_resize_spec_the_grids_are_whole(crops):
    e, geom, _ = tower("vit16")
    try:
        fit = e.pool_grids(crops[2])
        e.set_resize_spec("exact", 224, 2)
        assert e.pool_grids(crops[2]).tolist() == [[14, 14]] * N and fit.tolist() == [list(g) for g in GRIDS16]
        e.set_pooling("cls+mean")
        a32, a16 = e.embed(*crops)
        b32, b16 = e.vit_forward(e.preprocess(*crops))
        torch.cuda.synchronize()
        assert_bits(bits(a32), bits(b32), "resize spec: embed pools whole grids, f32")
        assert_bits(bits(a16), bits(b16), "resize spec: bf16")
        e.set_resize_rule("clip")
        assert e.pool_grids(crops[2]).tolist() == [[14, 14]] * N
        e.set_resize_rule("fit_pad")
        assert e.pool_grids(crops[2]).tolist() == fit.tolist()
        with pytest.raises(MmeError, match=r"mme_pool_grids: crop 1 has size 0x5"):
            e.pool_grids([[3, 3], [0, 5]])
    finally:
        e.close()


def test_mode_zero_is_untouched_and_a_load_resets_the_mode(crops):
    e, geom, w = tower("vit16")
    try:
        e.set_forward_pruning(True)
        patches = e.preprocess(*crops)

        def launches():
            e.profile(True)
            out = e.vit_forward(patches, pool_token=5)
            counts = {k: v[1] for k, v in e.profile_read().items()}
            e.profile(False)
            return out, counts

        (b32, b16), before = launches()
        assert e.pooling == "token" and e.embed_dim == D
        e.set_pooling("mean")
        e.profile(True)
        e.embed(*crops)
        mean_counts = {k: v[1] for k, v in e.profile_read().items()}
        e.profile(False)
        e.set_pooling("token")
        (a32, a16), after = launches()
        torch.cuda.synchronize()
        assert_bits(bits(a32), bits(b32), "a mode-0 forward after a mode-1 call, f32")
        assert_bits(bits(a16), bits(b16), "bf16")
        assert after == before, "the pruning setting is what it was: the same launches"
        e.set_forward_pruning(False)
        _, full = launches()
        assert full != before and mean_counts["pool"] == 3, (full, before, mean_counts)  # three chunks, one pooling launch each: unpruned
        e.set_pooling("cls+mean")
        assert e.embed_dim == 2 * D and e.encoder_info()["embed_dim"] == 2 * D
        e.load_vit(w, geom=geom)
        assert e.pooling == "token" and e.embed_dim == D
    finally:
        e.close()


def test_which_loads_reset_the_mode(crops):
    """Every image-tower load resets the mode, the tile tower's included; a text-tower load replaces the text tower and nothing
    of the image side (include/mme.h), so the mode and the vectors stay."""
    import dataclasses

    from multimodal_embeddings_amd.weights import TILE_VIT, CLIPTextGeometry, make_clip_text_weights, make_tile_vit_weights

    for key in ("dinov2", "vit32"):
        e, geom, w = tower(key)
        try:
            e.set_pooling("mean")
            getattr(e, TOWERS[key][0])(w, geom=geom)
            assert e.pooling == "token", key
        finally:
            e.close()
    e, geom, w = tower("vit16")
    try:
        e.set_pooling("cls+mean")
        b32, _ = e.embed(*crops)
        text = CLIPTextGeometry(num_layers=1, intermediate_size=64, vocab_size=96, eos_token_id=95)
        e.load_clip_text(make_clip_text_weights(3, text), text)
        assert e.pooling == "cls+mean" and e.embed_dim == 2 * D, "a text-tower load leaves the image side as it is"
        a32, _ = e.embed(*crops)
        torch.cuda.synchronize()
        assert_bits(bits(a32), bits(b32), "the vectors after a text-tower load")
        # a tile-tower load resets the mode although the ViT tower loaded before stays usable
        tile = dataclasses.replace(TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
        e.load_tile_vit(make_tile_vit_weights(5, tile), tile)
        assert e.pooling == "token" and e.embed_dim == D
        e.set_pooling("mean")  # the ViT tower is still loaded: the mean modes are accepted again
        assert e.pooling == "mean"
    finally:
        e.close()


def test_refusals_name_the_argument(crops):
    import dataclasses

    from multimodal_embeddings_amd.embedder import RegionEmbedder
    from multimodal_embeddings_amd.weights import TILE_VIT, make_tile_vit_weights

    bare = Engine(0)
    try:
        with pytest.raises(MmeError, match=r"mme_set_pooling: mode = 1 with encoder none loaded; supported: modes 1 and 2 with a vit or dinov2 tower loaded"):
            bare.set_pooling("mean")
        with pytest.raises(MmeError, match=r"mme_set_pooling: mode = 3; supported 0 \(MME_POOL_TOKEN\), 1 \(MME_POOL_MEAN\) and 2 \(MME_POOL_CLS_MEAN\)"):
            bare.set_pooling(3)
        with pytest.raises(MmeError, match="mme_set_pooling: mode = -1; supported 0"):
            bare.set_pooling(-1)
        bare.set_pooling("token")  # the default is accepted everywhere
        tile = dataclasses.replace(TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,))
        bare.load_tile_vit(make_tile_vit_weights(5, tile), tile)
        with pytest.raises(MmeError, match="mme_set_pooling: mode = 2 with encoder tile_vit; supported"):
            bare.set_pooling("cls+mean")
    finally:
        bare.close()
    for key, name in (("clip", "clip"), ("clip_proj", "clip"), ("siglip", "siglip")):
        loader, geom, make, _, _ = TOWERS[key]
        e = Engine(0)
        try:
            getattr(e, loader)(make(7, geom), geom=geom)
            with pytest.raises(MmeError, match=f"mme_set_pooling: mode = 1 with encoder {name}; supported"):
                e.set_pooling("mean")
            assert e.pooling == "token"
        finally:
            e.close()
    e, geom, _ = tower("vit16")
    try:
        patches = e.preprocess(*crops)
        with pytest.raises(MmeError, match=r"mme_vit_forward_grids: pooling mode 0 \(MME_POOL_TOKEN\); supported: 1 \(MME_POOL_MEAN\) and 2"):
            e.vit_forward(patches, grids=np.ones((N, 2), np.int32))
        e.set_pooling("mean")
        out = Guard(F32, N, D)
        for value, (i, j) in ((0, (2, 1)), (15, (4, 0)), (-1, (0, 0))):
            grids = np.full((N, 2), 14, np.int32)
            grids[i, j] = value
            rc = e.lib.mme_vit_forward_grids(e.h, patches.data_ptr(), N, grids.ctypes.data, out.view.data_ptr(), None, None)
            assert rc != 0 and f"mme_vit_forward_grids: grids[{i}][{j}] = {value}; supported 1..14".encode() in e.lib.mme_last_error(e.h)
        torch.cuda.synchronize()
        assert out.untouched(), "a refused call launched"
        with pytest.raises(ValueError, match="grids holds 2 rows for 6 crops"):
            e.vit_forward(patches, grids=np.ones((2, 2), np.int32))
    finally:
        e.close()
    with pytest.raises(ValueError, match=r"pool = 'mean': encoder='clip' pools .*supported: 'mean' and 'cls\+mean' with encoder='vit' and encoder='dinov2'"):
        RegionEmbedder(device=0, encoder="clip", pool="mean")
    with pytest.raises(ValueError, match="pool must be 'cls' or 'last'"):
        RegionEmbedder(device=0, encoder="vit", pool="max")


def test_region_embedder_returns_the_mean_pooled_vectors(crops):
    from multimodal_embeddings_amd.cross_compare import cross_compare
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    _, geom, make, T, first = TOWERS["vit16"]
    rng = np.random.default_rng(21)
    items = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES + [(300, 60), (224, 224), (77, 500)]]
    emb = RegionEmbedder(device=0, encoder="vit", weights=make(7, geom), geometry=geom, pool="cls+mean", chunk=4)
    try:
        assert emb.embed_dim == 768 and emb.pool == "cls+mean" and emb.pool_token == 0 and all(e.pooling == "cls+mean" for e in emb.engines)
        pix, offs, hw = emb.pack(items)
        want, want16 = emb.engine.embed(pix, offs, hw)
        torch.cuda.synchronize()
        vectors = emb.get_image_embeddings(items)
        got = torch.tensor(vectors, dtype=F32)
        assert tuple(got.shape) == (len(items), 768)
        assert_bits(bits(got), bits(want.cpu()), "get_image_embeddings against the engine call, in input order")
        p32, p16 = emb.embed_packed(pix, offs, hw)
        assert_bits(bits(p32), bits(want), "embed_packed")
        v2, tokens = emb.get_patch_embeddings(items)
        assert v2 == vectors and tuple(tokens.shape) == (len(items), T - first, D)
        emb.engine.set_pooling("token")
        tok0, _, _ = emb.engine.embed_tokens(pix, offs, hw)
        emb.engine.set_pooling("cls+mean")
        torch.cuda.synchronize()
        assert_bits(bits(tokens).view(len(items), -1), bits(tok0).view(len(items), -1), "the token blocks are those of mode 0")
        sim = cross_compare(want16, engine=emb.engine)  # 2 x hidden reaches K9
        rows = want16.double()
        assert tuple(sim.shape) == (len(items), len(items)) and float((sim.double() - rows @ rows.T).abs().max()) <= 2e-6
    finally:
        for e in emb.engines:
            e.close()
    mean = RegionEmbedder(device=0, encoder="dinov2", weights=TOWERS["dinov2"][2](7, TOWERS["dinov2"][1]), geometry=TOWERS["dinov2"][1], pool="mean", chunk=4)
    try:
        assert mean.embed_dim == D and mean.engine.pooling == "mean"
        u32, _ = mean.embed_uniform(torch.from_numpy(np.stack([items[0], items[7]])).to(DEV))
        pix, offs, hw = mean.pack([items[0], items[7]])
        w32, _ = mean.engine.embed(pix, offs, hw)
        torch.cuda.synchronize()
        assert_bits(bits(u32), bits(w32), "embed_uniform")
    finally:
        for e in mean.engines:
            e.close()


def test_forward_with_grids_runs_on_the_callers_stream():
    import stream_probes as sp

    loader, geom, make, _, _ = TOWERS["vit16"]

    def setup():
        e = Engine(0)
        getattr(e, loader)(make(7, geom), geom=geom)
        e.set_chunk(4)
        e.set_pooling("cls+mean")
        return e

    def inputs(v):
        g = torch.Generator().manual_seed(100 + v)
        rng = np.random.default_rng(200 + v)
        return {"patches": torch.randn((4 * 196, 768), generator=g).to(BF16)}, {"grids": rng.integers(1, 15, (4, 2)).astype(np.int32)}

    def call(e, d, h):
        return dict(zip(("e32", "e16"), e.vit_forward(d["patches"], grids=h["grids"])))

    case = sp.Case("vit_forward_grids", "vit_forward_grids-vit16", setup, inputs, call)
    bad_a, eff_a = sp.probe_a(case)
    bad_b, eff_b = sp.probe_b(case)
    print(f"vit_forward_grids: probe A effective {eff_a}, probe B effective {eff_b}")
    assert not bad_a and not bad_b, (bad_a, bad_b)
    assert eff_a or eff_b, "neither probe could have seen a violation"
