"""The five row kernels of the tile-ViT forward (csrc/tilevit.hip: tile_patchify, tile_assemble, tile_ln_post, tile_output,
tile_pool), one launch at a time (mme_tile_rowop_apply), against float64 written here from the definitions.

Reference: float64 on the device with torch, from the SAME bits the kernel reads, written from oracle/mllama_vision.py /
transformers' MllamaVisionModel (patch unfold in (c, ky, kx) order; class token | patch embedding + pre-tile embedding,
+ position embedding + tile position embedding, layernorm_pre, zero padding rows; layernorm_post + post-tile embedding
on every row; cat(final state, stack(states, dim=-1).flatten); class token of tile 0 / max(||.||, 1e-12)).  Nothing is
taken from kernel code.  Every output sits in a `Guard` of tests/test_gpu_gemm.py (helpers and sentinels are imported
from there): sentinel rows before and behind, pre-filled with the sentinel NaN pattern, which must be unchanged where
the kernel has nothing to write.  The kernels' row pitches (640, 1280, 1280 (1 + ni)) are the buffers' widths, so there
are no guard columns.  Row r of a padded sequence is (image, tile, tok) = (r // 6432, r // 1608 % 4, r % 1608).

(a) tile_patchify, bit for bit.  pv: uniform f32 in [-2.7, 2.7); a random half of the values has bit 15 set, so that
    three quarters of all values round away from zero (plain uniform data would leave the truncation mutant at 49.999 %).
    npatch = 1600 + 1603 reads three patches of a THIRD tile, so pv holds 3 tiles (2 would be read out of bounds).
    Planted in tile 1 by bit pattern: -0.0 -> 0x8000; 1 + 2^-8 (tie, down to even) -> 0x3F80; 1 + 3 2^-8 (tie, up to
    even) -> 0x3F82; 3.3e38 -> 0x7F78; 1e-39 (f32 subnormal, 0x000AE398) -> 0x000B, the RNE value 11 * 2^-133: that is
    what torch.Tensor.to(bfloat16) gives on the CPU and (asserted by the test) on the device; it is not flushed to zero.
    Want: pv viewed [tile, c, py, ky, px, kx] -> [tile, py, px, c, ky, kx], .to(bfloat16); columns 588..639 +0 bits.
    Mutants (bits differ on at least half of: all elements for the first three, the pad columns for the last): element
    order (ky, kx, c); px and py exchanged; truncation instead of RNE; the pad columns left as they were.
(b) tile_assemble.  aspect_rows 3, aid (2, 0, 1), rows = 2 * 6432 + 1608 + 3 (two images, tile 0 of the third, three
    rows of its tile 1), eps 1e-5.  pemb bf16 N(0, 1), cls N(0, 1), pre / pos / tilepos 0.5 N, gamma 1 + 0.2 N, beta 0.5 N.
    Families planted into the patch embeddings of tile 2 of image 0 (320 rows each): +30; one element 300; x 2^-20;
    x 2^20; constant rows (0, 1.5, -40; held to the tolerance).  One more family is this file's own: "near_eps", tokens
    1..320 of tile 3 of image 1 with pemb, pre, pos and tilepos of those rows x 2^-8, so that var(v) ~ 3e-5 is of the
    order of eps: the only rows on which a wrong eps shows through the bf16 rounding.
    v = (pemb + pre[aid, tile]) + pos[tok] + tilepos[aid, tile, tok] for tok >= 1, cls + pos[0] + tilepos[aid, tile, 0]
    for tok 0 (no pre); ref = two-pass LayerNorm(v) gamma + beta; rows with tok >= 1601 are +0 bits.
    tol = ulp_bf16(ref)/2 + (e (|v| + |mean|) + 3 2^-24 (|pemb| + |pre| + |pos| + |tilepos|)) rstd |gamma| + e |beta|
          + d_var / (2 (var + eps)) |ref - beta|,   d_var = e var + (e sum|v| / d)^2 + 2^-22 (var + eps),  e = 1280 2^-23
    (the two-pass bound of tests/test_gpu_gemm.py at d = 1280; no extra margin; a float32 numpy restatement of the
    definition reached at most 0.96 of it on the CPU, the half-ulp term dominating).
    Observed error / bound, maximum per family (MI355X, printed by the test, `pytest -s`):
    normal 0.961, class 0.960, +30 0.662, massive 0.960, x 2^-20 0.957, x 2^20 0.961, constant 0.956, near_eps 0.958.
    Mutants, on the normal-family rows (every real row outside tile 2 of image 0 and tile 3 of image 1), each more than
    4 x tol away on at least half of the elements of the rows it affects: pre added to the class row too; pre left out;
    aid of image 0 for every image; tile = it >> 2 and image = it & 3; pos[tok - 1] for pos[tok]; tilepos without the
    tile offset; (bits) padding rows normalised -- LayerNorm(0) = beta -- instead of zeroed.  This file's own: eps 1e-6
    and eps 1e-12 on the near_eps family; truncation instead of RNE leaves 1 x tol on more than a quarter of the
    normal-family elements (it cannot leave 4 x: its error is below one ulp).
    NOT separated, measured instead: variance as E[v^2] - mean^2 in f32 on the +30 family.  Emulated in float32 numpy in
    a kernel's order (20 values per lane, then the 64-lane tree) its relative rstd error is 1.1e-4, summed sequentially
    1.1e-3 (CPU, 400 rows), against the bf16 half-ulp of 2^-9 that every output carries: through a bf16 output no
    elementwise bound of this kind can tell it from the truth at an offset of 30, and a larger offset widens the
    e |mean| rstd term of the bound faster than the mutant's error grows against it.  The test runs the emulation on
    the device on its own +30 rows, prints the figures and asserts nothing about them.  Measured: relative rstd error
    9.9e-5, the mutant's unrounded output at most 0.027 x tol from the reference, 0 of 409600 elements beyond 4 x tol.
(c) tile_ln_post, in place.  Same aid and rows; x bf16 with the same families as rows of x (near_eps: x 2^-8); the
    padding rows of tiles (image 0, tile 0) and (image 1, tile 1) are all-zero, the others random: every row is normalised.
    ref = LN + post[aid, tile], LN = LayerNorm(x) gamma + beta;  tol = ulp_bf16(ref)/2 + e (|x| + |mean|) rstd |gamma|
    + e |beta| + d_var / (2 (var + eps)) |LN - beta| + 2^-23 (|LN| + |post|).  An all-zero row gives
    bf16_rne(f32(beta + post)) bit for bit; the rows >= `rows` of the buffer keep their contents bit for bit.
    Observed error / bound, maximum per family:
    normal 0.998, +30 0.649, massive 0.994, x 2^-20 0.999, x 2^20 0.995, constant 0.989, near_eps 0.995, all-zero 0.990,
    random padding rows 0.985.
    Mutants: post of tile 0 for every tile; aid of image 0; post added before gamma; padding rows skipped; eps 1e-6 /
    1e-12 on the near_eps family.
(d) tile_output, bit for bit (bf16 -> f32 widening).  ni 0 (inter NULL), 1, 5, 8; out_rows = 1601 + 5 (into tile 1, whose
    source rows skip the 7 padding rows); inter_stride = (2 * 1608 + 11) * 1280.  x / inter random bf16 with -0.0 and a
    bf16 subnormal planted.  Mutants (bits, at least half of the affected elements): layout k * 1280 + d (ni > 1);
    padding rows not skipped (rows of tile 1); inter_stride taken as 2 * 1608 * 1280 (states k >= 1).
(e) tile_pool.  n = 5 (image stride 4 * 1608 rows), ni 0 and 5.  Image 3's row is zero in x and every state: output
    exactly 0.  Image 4's row is scaled by 2^60: the sum of squares of such a row passes the f32 range (1280 * 2^120), so
    the kernel must scale before it squares; finite, unit norm.  bf16 output == RNE of the f32 output bit for bit; each
    output requested alone has the same bits; rows have unit norm to 1e-5; f32 output against float64 within 8 x the
    maximum deviation of a float32 numpy restatement of the definition, never below 2^-22 (the rule of test_pool_ln_l2).
    The restatement reads image 4's row BEFORE the scaling (a power of two: the same unit vector; plain f32 numpy
    overflows on the scaled row).  Measured (ni 0 / ni 5):
    float32 yardstick 5.28e-9 / 2.84e-9, tolerance 2.38e-7 (the 2^-22 floor) both, kernel maximum 8.82e-9 / 3.72e-9.
    Mutants (4 x tol, at least half of the elements of images 0, 1, 2): token 0 of tile 1 pooled; image stride 4 * 1601
    (images 1, 2); normalised over the first 1280 features only (ni 5).
(f) Argument validation: each documented precondition returns MME_E_ARG (MmeError) with its message and the
    sentinel-filled outputs stay untouched.  Only invalid-argument returns are exercised.
"""
import numpy as np
import pytest
import torch

from test_gpu_gemm import (BF16, DEV, F32, F64, SENT16, SENT32, Guard, _gen, _randn, assert_bits, assert_close, assert_mutant_bits,
                           assert_mutant_far, f32_eps, ulp_bf16)

pytestmark = pytest.mark.gpu

D, TOK, TOKP, TILES, GRID, PS, IMG = 1280, 1601, 1608, 4, 40, 14, 560
NPATCH = GRID * GRID        # 1600 patches per tile
PDIM, PDIMP = 588, 640      # 3 * 14 * 14 patch elements, the padded row of the patch matrix
SEQ = TILES * TOKP          # 6432 rows per image
E = D * 2.0**-23
EPS = 1e-5
AID = (2, 0, 1)
ROWS = 2 * SEQ + TOKP + 3
I16, I32 = torch.int16, torch.int32


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def _f32_bits(values):
    """int32 bit patterns of float32(values), made on the host (no device conversion in between)"""
    return torch.from_numpy(np.asarray(values, dtype=np.float32).view(np.int32).copy()).to(DEV)


def _dev(t):
    return torch.tensor(t, device=DEV)


def _rows(rows):
    """(it, tok, tile, image) of the padded-sequence rows 0 .. rows - 1"""
    r = torch.arange(rows, device=DEV)
    it = r // TOKP
    return it, r % TOKP, it % TILES, it // TILES


def _ln64(v, gamma, beta, eps):
    """two-pass LayerNorm from the definition -> (LN(v) gamma + beta, mean, var, rstd)"""
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    return (v - mean) * rstd * gamma + beta, mean, var, rstd


def _d_var(v, var, eps):
    return E * var + (E * v.abs().sum(1, keepdim=True) / D) ** 2 + 2.0**-22 * (var + eps)


def _report(what, got64, ref, tol, families):
    err = (got64 - ref).abs() / tol.clamp_min(1e-300)
    for name, idx in families.items():
        print(f"{what} family {name}: max err / bound = {float(err[idx].max()):.3g} ({idx.numel()} rows)")


def _family_rows(it0, count=320):
    """the five planted families as row indices: tokens 1 + 320 k .. 320 (k + 1) of tile `it0`"""
    base = it0 * TOKP + 1
    names = ("offset30", "massive", "small", "large", "constant")
    return {n: torch.arange(base + k * count, base + (k + 1) * count, device=DEV) for k, n in enumerate(names)}


def _plant_families(X, fam, g):
    """X f64 [*, D] standard normal rows; fam: {family: row indices into X}"""
    X[fam["offset30"]] += 30.0
    cols = torch.randint(0, D, (fam["massive"].numel(),), generator=g, device=DEV)
    X[fam["massive"], cols] = 300.0
    X[fam["small"]] *= 2.0**-20
    X[fam["large"]] *= 2.0**20
    consts = _dev([0.0, 1.5, -40.0]).double()
    X[fam["constant"]] = consts[torch.arange(fam["constant"].numel(), device=DEV) % 3][:, None]
    X[fam["near_eps"]] *= 2.0**-8


# ---------------------------------------------------------------------------------------------------------------------
# (a) tile_patchify


def test_tile_patchify_bit_for_bit(eng):
    g = _gen(11)
    tiles, npatch = 3, NPATCH + 1603
    pv = torch.rand((tiles, 3, IMG, IMG), generator=g, device=DEV) * 5.4 - 2.7
    bit15 = (torch.rand(pv.shape, generator=g, device=DEV) < 0.5).to(I32) * 0x8000
    pv.view(I32).bitwise_or_(bit15)
    planted = [-0.0, 1.0 + 2.0**-8, 1.0 + 3 * 2.0**-8, 1e-39, 3.3e38]
    where = [(1, 0, 0, 0), (1, 1, 5, 7), (1, 2, 100, 200), (1, 0, 559, 559), (1, 2, 300, 13)]
    pbits = _f32_bits(planted)
    assert pbits.tolist() == [-0x80000000, 0x3F808000, 0x3F818000, 0x000AE398, 0x7F7843B0]
    for b, w in zip(pbits, where):
        pv.view(I32)[w] = b
    # the reference conversion itself, on the device: RNE, ties to even, subnormals kept
    conv = pbits.view(F32).to(BF16).view(I16).to(I32) & 0xFFFF
    print("torch .to(bfloat16) of the planted values on the device:", [hex(v) for v in conv.tolist()])
    assert conv.tolist() == [0x8000, 0x3F80, 0x3F82, 0x000B, 0x7F78]
    out = Guard(BF16, npatch, PDIMP)
    eng.tile_rowop_apply("patchify", pv=pv, patches=out.view, npatch=npatch)
    out.check("tile_patchify")

    def unfold(order):
        return pv.view(tiles, 3, GRID, PS, GRID, PS).permute(*order).reshape(tiles * NPATCH, PDIM)[:npatch].contiguous()

    def padded(bits588, pad=0):
        w = torch.full((npatch, PDIMP), pad, dtype=I16, device=DEV)
        w[:, :PDIM] = bits588
        return w

    src = unfold((0, 2, 4, 1, 3, 5))  # [tile, py, px, c, ky, kx]
    want = padded(src.to(BF16).view(I16))
    assert_bits(out.valid_bits(), want, "tile_patchify")
    n = want.numel()
    assert_mutant_bits(padded(unfold((0, 2, 4, 3, 5, 1)).to(BF16).view(I16)), want, n // 2, "element order (ky, kx, c)")
    assert_mutant_bits(padded(unfold((0, 4, 2, 1, 3, 5)).to(BF16).view(I16)), want, n // 2, "px and py exchanged")
    assert_mutant_bits(padded((src.view(I32) >> 16).to(I16)), want, n // 2, "truncation instead of RNE")
    assert_mutant_bits(padded(want[:, :PDIM], SENT16)[:, PDIM:], want[:, PDIM:], npatch * (PDIMP - PDIM) // 2, "pad columns left as they were")


# ---------------------------------------------------------------------------------------------------------------------
# (b) tile_assemble


@pytest.fixture(scope="module")
def assemble_case():
    """inputs of (b): kernel tensors and their float64 copies, the families, the true reference with its tolerance"""
    g = _gen(21)
    eps = f32_eps(EPS)
    it, tok, tile, img = _rows(ROWS)
    real = tok < TOK
    npe = 9 * NPATCH + 2  # the last row read: (it 9, tok 2) -> patch row 9 * 1600 + 1
    P = torch.randn((npe, D), generator=g, device=DEV, dtype=F64)
    fam = _family_rows(2)
    fam["near_eps"] = torch.arange(7 * TOKP + 1, 7 * TOKP + 321, device=DEV)
    prow = lambda rows: (rows // TOKP) * NPATCH + rows % TOKP - 1  # noqa: E731  patch-embedding row of a padded-sequence row
    _plant_families(P, {k: prow(v) for k, v in fam.items()}, g)
    pemb = P.to(BF16)
    cls = _randn((D,), g)
    pre, pos, tilepos = _randn((3, TILES, D), g, 0.5), _randn((TOK, D), g, 0.5), _randn((3, TILES, TOK, D), g, 0.5)
    pre[0, 3] *= 2.0**-8  # image 1 has aid 0: (aid 0, tile 3) is the near_eps tile
    pos[1:321] *= 2.0**-8
    tilepos[0, 3, 1:321] *= 2.0**-8
    gamma, beta = (1.0 + _randn((D,), g, 0.2)).contiguous(), _randn((D,), g, 0.5)
    aid = _dev(list(AID) + [0]).to(I32)  # a fourth entry for the "image = it & 3" mutant only; the kernel reads three
    c = dict(pemb=pemb, cls=cls, pre=pre, pos=pos, tilepos=tilepos, gamma=gamma, beta=beta, aid=aid, eps=eps, fam=fam,
             it=it[real], tok=tok[real], tile=tile[real], img=img[real], real=real,
             f64={k: t.double() for k, t in dict(pemb=pemb, cls=cls, pre=pre, pos=pos, tilepos=tilepos, gamma=gamma, beta=beta).items()})
    normal = real & (it != 2) & (it != 7)
    fam["normal"] = normal.nonzero()[:, 0]
    fam["class"] = (tok == 0).nonzero()[:, 0]
    return c


def assemble_v(c, *, a=None, tile=None, pos_tok=None, tp_tile=None, pre="patch"):
    """v of every real row and its four terms (float64), with the index maps a mutant changes"""
    f, it, tok = c["f64"], c["it"], c["tok"]
    tile = c["tile"] if tile is None else tile
    a = c["aid"].long()[c["img"]] if a is None else a
    is_cls = (tok == 0)[:, None]
    first = torch.where(is_cls, f["cls"][None, :], f["pemb"][(it * NPATCH + tok - 1).clamp_min(0)])
    pr = f["pre"][a, tile]
    if pre == "none":
        pr = torch.zeros_like(pr)
    elif pre == "patch":
        pr = torch.where(is_cls, torch.zeros_like(pr), pr)
    po = f["pos"][tok if pos_tok is None else pos_tok]
    tp = f["tilepos"][a, tile if tp_tile is None else tp_tile, tok]
    return (first + pr) + po + tp, first, pr, po, tp


def assemble_ref(c, eps=None, **kw):
    v = assemble_v(c, **kw)[0]
    return _ln64(v, c["f64"]["gamma"], c["f64"]["beta"], c["eps"] if eps is None else eps)[0]


def test_tile_assemble(eng, assemble_case):
    c = assemble_case
    f, fam, real, eps = c["f64"], c["fam"], c["real"], c["eps"]
    x = Guard(BF16, ROWS, D)
    eng.tile_rowop_apply("assemble", pemb=c["pemb"], cls=c["cls"], pre=c["pre"], pos=c["pos"], tilepos=c["tilepos"], gamma=c["gamma"], beta=c["beta"],
                         aid=c["aid"], x=x.view, rows=ROWS, eps=EPS, aspect_rows=3)
    x.check("tile_assemble")
    got_bits = x.valid_bits()
    assert bool((got_bits[~real] == 0).all()), "tile_assemble: a padding row (tok >= 1601) is not +0 bits"
    v, first, pr, po, tp = assemble_v(c)
    ref, mean, var, rstd = _ln64(v, f["gamma"], f["beta"], eps)
    tol = (ulp_bf16(ref) / 2 + (E * (v.abs() + mean.abs()) + 3 * 2.0**-24 * (first.abs() + pr.abs() + po.abs() + tp.abs())) * rstd * f["gamma"].abs()
           + E * f["beta"].abs() + _d_var(v, var, eps) / (2 * (var + eps)) * (ref - f["beta"]).abs())
    del first, pr, po, tp
    # positions among the real rows of the families' padded-sequence rows
    pos_of = torch.cumsum(real.long(), 0) - 1
    sel = {k: pos_of[r] for k, r in fam.items()}
    got = x.valid[real].double()
    _report("tile_assemble", got, ref, tol, sel)
    assert_close(got, ref, tol, "tile_assemble")

    # ---- mutants on the normal-family rows
    nrm = torch.zeros(ref.shape[0], dtype=torch.bool, device=DEV)
    nrm[sel["normal"]] = True
    it, tok, tile, img = c["it"], c["tok"], c["tile"], c["img"]
    a_true = c["aid"].long()[img]

    def far(name, affected, **kw):
        m = nrm & affected
        assert int(m.sum()) > 0
        mut = assemble_ref(c, **kw)
        assert_mutant_far(mut[m], ref[m], tol[m], int(m.sum()) * D // 2, name)

    far("pre added to the class row too", tok == 0, pre="all")
    far("pre left out", tok > 0, pre="none")
    far("aid of image 0 for every image", img > 0, a=torch.full_like(a_true, AID[0]))
    t_mut, i_mut = it >> 2, it & 3
    far("tile = it >> 2, image = it & 3", (t_mut != tile) | (i_mut != img), a=c["aid"].long()[i_mut], tile=t_mut)
    far("pos[tok - 1] for pos[tok]", tok > 0, pos_tok=(tok - 1).clamp_min(0))
    far("tilepos without the tile offset", tile > 0, tp_tile=torch.zeros_like(tile))
    pad_rows = int((~real).sum())
    assert_mutant_bits(c["beta"].to(BF16).view(I16)[None, :].expand(pad_rows, D), got_bits[~real], pad_rows * D // 2, "padding rows normalised instead of zeroed")
    ne = torch.zeros_like(nrm)
    ne[sel["near_eps"]] = True
    for wrong in (1e-6, 1e-12):
        mut = assemble_ref(c, eps=f32_eps(wrong))
        assert_mutant_far(mut[ne], ref[ne], tol[ne], int(ne.sum()) * D // 2, f"eps {wrong:g}")
    trunc = ((ref[nrm].float().view(I32) >> 16) << 16).view(F32).double()
    n_tr = int(((trunc - ref[nrm]).abs() > tol[nrm]).sum())
    assert n_tr >= int(nrm.sum()) * D // 4, f"mutant 'truncation instead of RNE' leaves the tolerance on {n_tr} elements only"
    # ---- measured, not asserted (module docstring): variance as E[v^2] - mean^2 in f32, a kernel's order, on the +30 rows
    o = sel["offset30"]
    v32 = v[o].float()
    lanes = v32.view(-1, 5, 64, 4).permute(0, 2, 1, 3).reshape(-1, 64, 20)

    def lane_sum(t):
        s = torch.zeros(t.shape[:2], dtype=F32, device=DEV)
        for j in range(20):
            s = s + t[:, :, j]
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
        return s

    m32 = lane_sum(lanes) * np.float32(1.0 / D)
    var32 = lane_sum(lanes * lanes) * np.float32(1.0 / D) - m32 * m32
    mut = (v[o] - m32.double()) * (var32.double() + eps) ** -0.5 * f["gamma"] + f["beta"]
    print(f"tile_assemble mutant 'variance as E[v^2] - mean^2 in f32' on the +30 family: relative rstd error "
          f"{float(((var32.double() - var[o]).abs() / (2 * var[o])).max()):.3g}, max deviation / tol {float(((mut - ref[o]).abs() / tol[o]).max()):.3g}, "
          f"beyond 4 x tol on {int(((mut - ref[o]).abs() > 4 * tol[o]).sum())} of {mut.numel()} elements")


# ---------------------------------------------------------------------------------------------------------------------
# (c) tile_ln_post


def test_tile_ln_post(eng):
    g = _gen(31)
    eps = f32_eps(EPS)
    extra = 5  # rows behind `rows` inside the buffer: they keep their contents
    it, tok, tile, img = _rows(ROWS)
    X = torch.randn((ROWS + extra, D), generator=g, device=DEV, dtype=F64)
    fam = _family_rows(2)
    fam["near_eps"] = torch.arange(7 * TOKP + 1, 7 * TOKP + 321, device=DEV)
    _plant_families(X, fam, g)
    pad = tok >= TOK
    zero_rows = (pad & ((it == 0) | (it == 5))).nonzero()[:, 0]
    X[zero_rows] = 0.0
    fam["zero"] = zero_rows
    fam["padding"] = (pad & (it != 0) & (it != 5)).nonzero()[:, 0]
    fam["normal"] = (~pad & (it != 2) & (it != 7)).nonzero()[:, 0]
    xb = X.to(BF16)
    gamma, beta = (1.0 + _randn((D,), g, 0.2)).contiguous(), _randn((D,), g, 0.5)
    post = _randn((3, TILES, D), g, 0.5)
    aid = _dev(list(AID)).to(I32)
    buf = Guard(BF16, ROWS + extra, D)
    buf.valid.copy_(xb)
    eng.tile_rowop_apply("ln_post", x=buf.view, gamma=gamma, beta=beta, post=post, aid=aid, rows=ROWS, eps=EPS, aspect_rows=3)
    buf.check("tile_ln_post")
    assert_bits(buf.valid_bits()[ROWS:], xb.view(I16)[ROWS:], "tile_ln_post: rows >= `rows` must keep their contents")
    x, g64, b64, p64 = xb[:ROWS].double(), gamma.double(), beta.double(), post.double()
    a = aid.long()[img]
    ln, mean, var, rstd = _ln64(x, g64, b64, eps)
    po = p64[a, tile]
    ref = ln + po
    tol = (ulp_bf16(ref) / 2 + E * (x.abs() + mean.abs()) * rstd * g64.abs() + E * b64.abs() + _d_var(x, var, eps) / (2 * (var + eps)) * (ln - b64).abs()
           + 2.0**-23 * (ln.abs() + po.abs()))
    got = buf.valid[:ROWS].double()
    _report("tile_ln_post", got, ref, tol, fam)
    assert_close(got, ref, tol, "tile_ln_post")
    want_zero = (beta[None, :] + post[a[zero_rows], tile[zero_rows]]).to(BF16).view(I16)  # one f32 addition, then RNE
    assert_bits(buf.valid_bits()[zero_rows], want_zero, "tile_ln_post: all-zero rows")

    # ---- mutants
    nrm = torch.zeros(ROWS, dtype=torch.bool, device=DEV)
    nrm[fam["normal"]] = True
    nrm[fam["padding"]] = True

    def far(name, m, mut):
        assert int(m.sum()) > 0
        assert_mutant_far(mut[m], ref[m], tol[m], int(m.sum()) * D // 2, name)

    far("post of tile 0 for every tile", nrm & (tile > 0), ln + p64[a, torch.zeros_like(tile)])
    far("aid of image 0 for every image", nrm & (img > 0), ln + p64[torch.full_like(a, AID[0]), tile])
    far("post added before gamma", nrm, ((x - mean) * rstd + po) * g64 + b64)
    allpad = torch.zeros_like(nrm)
    allpad[fam["padding"]] = True
    allpad[zero_rows] = True
    far("padding rows skipped", allpad, x)
    ne = torch.zeros_like(nrm)
    ne[fam["near_eps"]] = True
    for wrong in (1e-6, 1e-12):
        far(f"eps {wrong:g}", ne, _ln64(x, g64, b64, f32_eps(wrong))[0] + po)


# ---------------------------------------------------------------------------------------------------------------------
# (d) tile_output


def _planted_bf16(shape, g):
    t = _randn(shape, g, 1.0, BF16)
    flat = t.view(-1).view(I16)
    flat[5] = -0x8000   # -0.0
    flat[D + 9] = 0x0003  # a bf16 subnormal
    flat[-1] = -0x7FFD  # a negative subnormal (0x8003)
    return t


@pytest.mark.parametrize("ni", [0, 1, 5, 8])
def test_tile_output_bit_for_bit(eng, ni):
    g = _gen(40 + ni)
    out_rows = TOK + 5
    ws_rows = 2 * TOKP + 11
    stride = ws_rows * D
    x = _planted_bf16((ws_rows, D), g)
    inter = _planted_bf16((ni, ws_rows, D), g) if ni else None
    F = D * (1 + ni)
    hid = Guard(F32, out_rows, F)
    eng.tile_rowop_apply("output", x=x, inter=inter, ni=ni, inter_stride=stride, hidden=hid.view, out_rows=out_rows)
    hid.check("tile_output")
    o = torch.arange(out_rows, device=DEV)
    src = (o // TOK) * TOKP + o % TOK  # the 7 padding rows of tile 0 are skipped

    def gather(rows, states=None, layout="dk"):
        parts = [x[rows].float()]
        if ni:
            st = (inter if states is None else states)[:, rows].float()  # [ni, R, D]
            parts.append((st.permute(1, 2, 0) if layout == "dk" else st.permute(1, 0, 2)).reshape(rows.numel(), D * ni))
        return torch.cat(parts, 1).view(I32)

    want = gather(src)
    assert_bits(hid.valid_bits(), want, f"tile_output ni {ni}")
    tail = o >= TOK
    assert_mutant_bits(gather(o)[tail], want[tail], int(tail.sum()) * F // 2, "padding rows not skipped")
    if ni > 1:
        assert_mutant_bits(gather(src, layout="kd")[:, D:], want[:, D:], out_rows * D * ni // 2, "layout k * 1280 + d")
        short = 2 * TOKP  # the mutant's stride: the rows of two tiles instead of the workspace's
        flat = inter.view(-1)
        st = torch.stack([flat[k * short * D : (k * short + short) * D].view(short, D) for k in range(ni)])
        assert_mutant_bits(gather(src, states=st)[:, D:], want[:, D:], out_rows * D * (ni - 1) // 2, "inter_stride taken as rows * 1280")


# ---------------------------------------------------------------------------------------------------------------------
# (e) tile_pool


def pool_ref(rows, dtype):
    """numpy restatement of the definition in `dtype`: x / max(||x||, 1e-12)"""
    r = rows.astype(dtype)
    nrm = np.sqrt((r * r).sum(1, keepdims=True, dtype=dtype))
    return r / np.maximum(nrm, dtype(1e-12))


@pytest.mark.parametrize("ni", [0, 5])
def test_tile_pool(eng, ni):
    g = _gen(50 + ni)
    n = 5
    R = (n - 1) * SEQ + 3
    F = D * (1 + ni)
    S = torch.randn((1 + ni, R, D), generator=g, device=DEV, dtype=F32)
    before = S[:, 4 * SEQ].clone()  # image 4's row before its scaling
    S[:, 3 * SEQ] = 0.0
    S[:, 4 * SEQ] *= 2.0**60
    S = S.to(BF16)
    x, inter = S[0], (S[1:] if ni else None)

    def feats(rows):
        """[len(rows), F] float64: x, then feature 1280 + d * ni + k = state k at dimension d"""
        parts = [S[0, rows].double()]
        if ni:
            parts.append(S[1:, rows].double().permute(1, 2, 0).reshape(rows.numel(), D * ni))
        return torch.cat(parts, 1)

    e32, e16 = Guard(F32, n, F), Guard(BF16, n, F)
    eng.tile_rowop_apply("pool", x=x, inter=inter, ni=ni, inter_stride=R * D, n=n, emb_f32=e32.view, emb_bf16=e16.view)
    e32.check("tile_pool f32")
    e16.check("tile_pool bf16")
    got = e32.valid.clone()
    assert bool(torch.isfinite(got).all()), "tile_pool: non-finite output"
    assert_bits(e16.valid_bits(), got.to(BF16).view(I16), "tile_pool: bf16 output vs RNE of the f32 output")
    assert bool((got[3] == 0).all()), "tile_pool: the all-zero row must give exactly 0"
    rows = torch.arange(n, device=DEV) * SEQ
    v = feats(rows).cpu().numpy()
    ref = pool_ref(v, np.float64)
    v_unscaled = v.copy()
    v_unscaled[4] = np.concatenate([before[0].to(BF16).double().cpu().numpy()] + ([before[1:].to(BF16).double().cpu().numpy().T.reshape(-1)] if ni else []))
    assert np.array_equal(v_unscaled[4] * 2.0**60, v[4])
    yard = float(np.abs(pool_ref(v_unscaled, np.float32).astype(np.float64) - ref).max())
    tol = max(8 * yard, 2.0**-22)
    g64 = got.double().cpu().numpy()
    err = float(np.abs(g64 - ref).max())
    print(f"tile_pool ni {ni}: float32 yardstick {yard:.3g}, kernel max deviation {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, f"tile_pool ni {ni}: max deviation {err:.3g} > {tol:.3g} (float32 yardstick {yard:.3g})"
    norms = np.linalg.norm(g64, axis=1)
    keep = np.array([0, 1, 2, 4])
    assert np.abs(norms[keep] - 1.0).max() <= 1e-5, f"tile_pool: row norms {norms}"
    # each output requested alone: the same bits
    o32, o16 = Guard(F32, n, F), Guard(BF16, n, F)
    eng.tile_rowop_apply("pool", x=x, inter=inter, ni=ni, inter_stride=R * D, n=n, emb_f32=o32.view)
    eng.tile_rowop_apply("pool", x=x, inter=inter, ni=ni, inter_stride=R * D, n=n, emb_bf16=o16.view)
    o32.check("tile_pool f32 alone")
    o16.check("tile_pool bf16 alone")
    assert torch.equal(o32.valid_bits(), e32.valid_bits()) and torch.equal(o16.valid_bits(), e16.valid_bits())
    # mutants
    sub = np.array([0, 1, 2])

    def far(name, mut, which=sub):
        k = int((np.abs(mut[which] - ref[which]) > 4 * tol).sum())
        assert k >= len(which) * F // 2, f"mutant '{name}' leaves 4 x the tolerance on {k} elements only"

    far("token 0 of tile 1 pooled", pool_ref(feats(rows[:4] + TOKP).cpu().numpy(), np.float64))
    far("image stride 4 * 1601", pool_ref(feats(torch.arange(4, device=DEV) * TILES * TOK).cpu().numpy(), np.float64), np.array([1, 2]))
    if ni:
        far("normalised over the first 1280 features only", v / np.linalg.norm(v[:, :D], axis=1, keepdims=True).clip(1e-12))


# ---------------------------------------------------------------------------------------------------------------------
# (f) argument validation: MME_E_ARG with its message, nothing launched


def test_tile_rowop_apply_refuses_bad_arguments(eng):
    from multimodal_embeddings_amd._lib import MmeError

    rows = 8
    vec = torch.zeros(D + 4, dtype=F32, device=DEV)
    tab = torch.zeros((TILES * D + 4,), dtype=F32, device=DEV)       # pre / post of one aspect row
    big = torch.zeros((TILES * TOK * D + 4,), dtype=F32, device=DEV)  # pos, and tilepos of one aspect row
    pv = torch.zeros((3 * IMG * IMG + 4,), dtype=F32, device=DEV)
    pemb = torch.zeros((rows * D + 8,), dtype=BF16, device=DEV)
    xin = torch.zeros((2 * TOKP * D + 8,), dtype=BF16, device=DEV)  # ops 3, 4 read it
    inter = torch.zeros((2 * 2 * TOKP * D + 8,), dtype=BF16, device=DEV)
    aid = torch.zeros(4, dtype=I32, device=DEV)
    aid_bad = _dev([0, 1, 0, 0]).to(I32)
    patches, x = Guard(BF16, rows, PDIMP), Guard(BF16, 2 * SEQ, D)
    hidden, e32, e16 = Guard(F32, rows, 3 * D), Guard(F32, 2, 3 * D), Guard(BF16, 2, 3 * D)
    outs = (patches, x, hidden, e32, e16)
    ok = {
        "patchify": dict(pv=pv[: 3 * IMG * IMG], patches=patches.view, npatch=rows),
        "assemble": dict(pemb=pemb[: rows * D], cls=vec[:D], pre=tab[: TILES * D], pos=big[: TOK * D], tilepos=big[: TILES * TOK * D], gamma=vec[:D],
                         beta=vec[:D], aid=aid, x=x.view, rows=rows, aspect_rows=1),
        "ln_post": dict(x=x.view, gamma=vec[:D], beta=vec[:D], post=tab[: TILES * D], aid=aid, rows=rows, aspect_rows=1),
        "output": dict(x=xin[: 2 * TOKP * D], inter=inter[: 2 * 2 * TOKP * D], ni=2, inter_stride=2 * TOKP * D, hidden=hidden.view, out_rows=rows),
        "pool": dict(x=xin[: 2 * TOKP * D], inter=inter[: 2 * 2 * TOKP * D], ni=2, inter_stride=2 * TOKP * D, n=1, emb_f32=e32.view, emb_bf16=e16.view),
    }

    def call(op, **over):
        kw = dict(ok.get(op, {}))
        kw.update(over)
        return lambda: eng.tile_rowop_apply(op, **kw)

    x16 = x.raw.view(BF16)
    bad = [
        (call(5), "op 5 outside"),
        (call(-1), "op -1 outside"),
        (call("patchify", pv=None), "op 0 needs pv, patches"),
        (call("patchify", patches=None), "op 0 needs pv, patches"),
        (call("patchify", pv=pv[1:]), "16-byte aligned"),
        (call("patchify", patches=patches.raw.view(BF16)[4:]), "16-byte aligned"),
        (call("patchify", npatch=-1), "npatch"),
        (call("patchify", npatch=2**31), "npatch"),
        (call("assemble", pemb=None), "op 1 needs pemb"),
        (call("assemble", cls=None), "op 1 needs pemb"),
        (call("assemble", pre=tab[1 : TILES * D + 1]), "op 1 needs pemb"),
        (call("assemble", pos=None), "op 1 needs pemb"),
        (call("assemble", tilepos=big[2:]), "op 1 needs pemb"),
        (call("assemble", gamma=None), "op 1 needs pemb"),
        (call("assemble", beta=vec[1 : D + 1]), "op 1 needs pemb"),
        (call("assemble", x=None), "op 1 needs pemb"),
        (call("assemble", x=x16[4:]), "op 1 needs pemb"),
        (call("assemble", pemb=pemb[4:]), "op 1 needs pemb"),
        (call("assemble", aid=None), "aid non-null"),
        (call("assemble", rows=-1), "rows"),
        (call("assemble", aspect_rows=0), "aspect_rows in 1..9"),
        (call("assemble", aspect_rows=10), "aspect_rows in 1..9"),
        (call("assemble", aid=aid_bad, rows=SEQ + 1), "aid[1] = 1 outside 0..0"),
        (call("ln_post", x=None), "op 2 needs x"),
        (call("ln_post", post=None), "op 2 needs x"),
        (call("ln_post", post=tab[1 : TILES * D + 1]), "op 2 needs x"),
        (call("ln_post", gamma=vec[2 : D + 2]), "op 2 needs x"),
        (call("ln_post", aid=None), "aid non-null"),
        (call("ln_post", rows=-5), "rows"),
        (call("ln_post", aspect_rows=0), "aspect_rows in 1..9"),
        (call("ln_post", aid=aid_bad, rows=SEQ + 1), "aid[1] = 1 outside 0..0"),
        (call("ln_post", aid=_dev([-1]).to(I32)), "aid[0] = -1 outside"),
        (call("output", x=None), "op 3 needs x, hidden"),
        (call("output", hidden=None), "op 3 needs x, hidden"),
        (call("output", hidden=hidden.raw.view(F32)[1:]), "op 3 needs x, hidden"),
        (call("output", out_rows=-1), "out_rows"),
        (call("output", ni=9), "ni in 0..8"),
        (call("output", ni=-1), "ni in 0..8"),
        (call("output", inter=None), "inter null exactly when ni == 0"),
        (call("output", ni=0), "inter null exactly when ni == 0"),
        (call("output", inter=inter[4:]), "inter 16-byte aligned"),
        (call("output", inter_stride=rows * D - 1), "inter_stride"),
        (call("output", out_rows=TOK + 1, inter_stride=(TOKP + 1) * D - 1), "inter_stride"),
        (call("output", inter_stride=2**40 + 1), "inter_stride"),
        (call("pool", x=xin[4:]), "op 4 needs x"),
        (call("pool", emb_f32=None, emb_bf16=None), "emb_f32 or emb_bf16"),
        (call("pool", emb_f32=e32.raw.view(F32)[1:]), "emb_f32 and emb_bf16 16-byte aligned"),
        (call("pool", emb_bf16=e16.raw.view(BF16)[4:]), "emb_f32 and emb_bf16 16-byte aligned"),
        (call("pool", n=-1), "n >= 0"),
        (call("pool", ni=9), "ni in 0..8"),
        (call("pool", inter=None), "inter null exactly when ni == 0"),
        (call("pool", n=2, inter_stride=SEQ * D), "inter_stride"),
    ]
    for fn, msg in bad:
        with pytest.raises(MmeError) as ei:
            fn()
        assert "(-1)" in str(ei.value) and msg in str(ei.value), f"expected MME_E_ARG with '{msg}', got: {ei.value}"
        assert all(o.untouched() for o in outs), f"a refused call ('{msg}') wrote to its output"
    # a count of 0 is MME_OK without a launch
    for op, count in (("patchify", "npatch"), ("assemble", "rows"), ("ln_post", "rows"), ("output", "out_rows"), ("pool", "n")):
        call(op, **{count: 0})()
        assert all(o.untouched() for o in outs), f"{op} with {count} = 0 wrote to its output"
    # the same arguments without the fault are accepted (the refusals above are not artefacts of the set-up)
    for op in ok:
        call(op)()
    call("output", ni=0, inter=None)()
    call("pool", ni=0, inter=None, emb_f32=None)()
