"""The 384 x 256 GEMM kernel (variant 6, csrc/gemm384r.hip) where tests/test_gpu_gemm384.py does not reach: its request
stream across more than two output tiles per workgroup, several column groups, the automatic choice at its threshold and
the product configuration end to end.  Every comparison is bit for bit: against float64 exact values, or against variant 3.

Geometry: the grid is min(tiles, 256) workgroups, tiles are 384 x 256, nk = K / 64 K-tiles, workgroup w runs tiles w,
w + 256, ...; the column tiles are walked in groups of gn = min(tiles_n, max(3, 4800 / K)) (csrc/gemm_tiles.h).

(A) The stream, exact (the family of tests/test_gpu_gemm.py (a): integer operands, sum |a w| < 2^24 asserted per element
    from the float64 pass, expected bits bf16_rne(exact value), every element compared, outputs and planes between
    sentinel guards).  Each shape is the smallest with its tile counts:
      A1  22 105 x 2304 x 768, epilogue 5, upwards (the QKV shape).  58 x 9 = 522 tiles (522 % 8 = 2: xcd_remap's ragged
          tail on a full grid): every workgroup runs two tiles, ten run three, so a tile is both entered from a previous one
          and followed by another; column groups 6 + 3 (a ragged last group); nk = 12; the ragged last row tile (217 rows)
          is prefetched across the stream from an interior tile.
      A2  65 764 x 768 x 3072, epilogue 8 with planes, entries in -1..1, residual in place, downwards (the fc2 shape).
          172 x 3 = 516 tiles; nk = 48; the ragged tile (100 rows) comes FIRST in its workgroups' order and interior tiles
          are prefetched from it -- the direction in which a look-ahead clamped with the current tile's extent changes
          stored values.  Planes: rows [0, 65 664) equal expected_planes of the expected output in bits, the rest sentinel.
      A3  24 793 x 1856 x 832, epilogue 2 out of place, upwards.  65 x 8 = 520 tiles; nk = 13 is odd, so every following
          tile's K-tile 0 sits in the LDS buffer the prologue does not use; gn = 5: groups 5 + 3, the last holding the
          64-column ragged tile (prefetched with another column clamp than its predecessor's).
      A4  147 840 x 512 x K, K = 128, 192, 320, epilogue 0, downwards.  385 x 2 = 770 tiles: every workgroup runs three
          tiles, two run four (steady state); nk = 2, 3, 5: at nk = 2 both look-aheads cross a tile boundary at every K-tile.
    Sharpness on A1 to A3, each mutant a change of the reference that must differ from the expected bits on at least half
    of the elements it touches: K-tile t of A (then of W) replaced by K-tile t - 2, which shares its ring buffer (a slot
    read before its refill landed); A[:, :64] rolled by 384 rows (the first K-tile fetched from the previous row panel);
    on A2, rows 100..383 of an interior row panel reading that panel's row 99 in the first K-tile (the look-ahead clamped
    with the ragged tile's extent).
    GELU has no exact family: fc1's shape, 16 345 x 3072 x 768 (43 x 12 = 516 tiles, groups 6 + 6), under epilogues 1 and 6
    on random data, variant 6 against variant 3 in bits.
(B) The automatic choice.  include/mme.h: variant 0 takes the 384 x 256 kernel for QKV, fc1 and fc2 of ViT-B from
    ceil(M / 384) (N / 256) >= 16 * 256 tiles on, else variant 4.  Epilogue 8 leaves planes for the rows of the interior row
    tiles of the kernel that ran, so the rows between the 256-row interior and the 384-row interior tell which one did: all
    sentinel at the last M below the threshold, all written at the first M at it, where output and common plane rows also
    equal an explicit variant 3 launch in bits.  o_proj's shape (768 x 768) stays on the 256-row kernel at 524 161 rows.
    Operands are drawn directly in bf16 (the largest A is 3.2 GB) and one allocation serves both values of M.
(D) The product configuration once: a two-layer ViT-B/16, 2700 crops in one chunk (531 900 token rows, above all three
    thresholds of (B)), variant 0 and variant 4 under LayerNorm fusion 2 and 1: four embedding tables equal in bits and
    finite.  (Variant 0 then runs QKV, fc1 and fc2 on the 384-row kernel, o_proj on the 256-row one, and splits every
    LayerNorm's rows into planes and x by the interior of the kernel that produced them.)
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_gemm import (BF16, DEV, F32, SENT32, Guard, _gen, acc64, assert_bits, assert_mutant_bits, exact_inputs,  # noqa: E402, F401
                           exact_value, expected_bits, expected_planes, launch)
from test_gpu_gemm384 import _data, _launch  # noqa: E402

TM, TN, TK, GRID = 384, 256, 64, 256


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def geometry(M, N, K):
    """(row tiles, column tiles, column groups, K-tiles, tiles of the busiest workgroup, workgroups that run that many)"""
    tm, tn, nk = -(-M // TM), -(-N // TN), K // TK
    gn = min(tn, max(3, 4800 // K))
    groups = [min(gn, tn - c) for c in range(0, tn, gn)]
    most = -(-(tm * tn) // GRID)
    return tm, tn, groups, nk, most, tm * tn - (most - 1) * GRID


# ---------------------------------------------------------------------------------------------------------------------
# (A) the stream across tiles

# name: (M, N, K, epilogue, reverse_m, residual in place, amax, planes, K-tile of the ring mutants, expected geometry)
STREAM = {
    "A1-qkv": (22105, 2304, 768, 5, 0, True, 3, False, 5, (58, 9, [6, 3], 12, 3, 10)),
    "A2-fc2": (65764, 768, 3072, 8, 1, True, 1, True, 47, (172, 3, [3], 48, 3, 4)),
    "A3-odd-nk": (24793, 1856, 832, 2, 0, False, 3, False, 12, (65, 8, [5, 3], 13, 3, 8)),
    "A4-nk2": (147840, 512, 128, 0, 1, True, 3, False, None, (385, 2, [2], 2, 4, 2)),
    "A4-nk3": (147840, 512, 192, 0, 1, True, 3, False, None, (385, 2, [2], 3, 4, 2)),
    "A4-nk5": (147840, 512, 320, 0, 1, True, 3, False, None, (385, 2, [2], 5, 4, 2)),
}


@pytest.mark.parametrize("name", list(STREAM))
def test_stream_exact_bit_for_bit(eng, name):
    M, N, K, epi, rev, inplace, amax, planes_on, tmut, geo = STREAM[name]
    assert geometry(M, N, K) == geo, geometry(M, N, K)
    what = f"stream {name}: epilogue {epi} M {M} N {N} K {K} reverse {rev}"
    d = exact_inputs(epi, M, N, K, 38400 + M + 7 * N + 13 * K + epi, amax=amax)
    A, W = d["A"], d["W"]
    acc = acc64(A, W)
    value = exact_value(epi, d, acc=acc)  # asserts sum |a w| < 2^24 per element
    want = expected_bits(epi, d, value, what)
    out, planes, ran = launch(eng, epi, A, W, 6, reverse_m=rev, bias=d.get("bias"), res=d.get("res"), inplace=inplace,
                              ln_stats=d.get("ln_stats"), colsum=d.get("colsum"), planes=planes_on, what=what)
    assert ran, f"{what}: a large-tile kernel must run"
    assert_bits(out.view(torch.int16), want, what)
    if planes_on:
        r6 = M // TM * TM
        pb = planes.view(torch.int32)
        wp = expected_planes(want, torch.arange(r6, device=DEV), what).view(torch.int32)
        assert_bits(pb[:, :, :r6].contiguous().flatten(0, 1), wp.flatten(0, 1), what + " planes")
        assert bool((pb[:, :, r6:] == SENT32).all()), f"{what}: planes written outside the interior row tiles"
    if tmut is None:
        return
    # ---- sharpness: each mutant is a change of the reference
    del out, planes
    half = want.numel() // 2
    kt, ks = slice(TK * tmut, TK * tmut + TK), slice(TK * (tmut - 2), TK * (tmut - 2) + TK)
    At, Wt = A[:, kt].double(), W[:, kt].double()

    def mutant(delta):
        return expected_bits(epi, d, exact_value(epi, d, acc=acc + delta), what)

    assert_mutant_bits(mutant((A[:, ks].double() - At) @ Wt.T), want, half, f"K-tile {tmut} of A read as K-tile {tmut - 2} (ring slot read before its refill)")
    assert_mutant_bits(mutant(At @ (W[:, ks].double() - Wt).T), want, half, f"K-tile {tmut} of W read as K-tile {tmut - 2} (ring slot read before its refill)")
    A0, W0 = A[:, :TK].double(), W[:, :TK].double()
    assert_mutant_bits(mutant((torch.roll(A0, TM, 0) - A0) @ W0.T), want, half, "first K-tile fetched from the previous row panel")
    if name == "A2-fc2":  # the panel the ragged tile's workgroups run next to it, its rows past the ragged extent clamped to row 99
        r0 = (M // TM - 1) * TM
        rag = M - M // TM * TM
        assert rag == 100
        sub = dict(d, A=A[r0 : r0 + TM].clone(), res=d["res"][r0 : r0 + TM])
        sub["A"][rag:, :TK] = A[r0 + rag - 1, :TK]
        mut = expected_bits(epi, sub, exact_value(epi, sub), what)
        assert_mutant_bits(mut[rag:], want[r0 + rag : r0 + TM], (TM - rag) * N // 2, "look-ahead clamped with the ragged tile's extent")


@pytest.mark.parametrize("epi", [1, 6])
def test_fc1_shape_gelu_equals_variant3_in_bits(eng, epi):
    M, N, K = 16345, 3072, 768
    assert geometry(M, N, K) == (43, 12, [6, 6], 12, 3, 4)
    d = _data(M, N, K)
    what = f"fc1 shape, epilogue {epi} M {M} N {N} K {K}"
    want, _ = _launch(eng, epi, d, 3, 0, True, what + " variant 3")
    got, _ = _launch(eng, epi, d, 6, 0, True, what + " variant 6")
    assert_bits(got, want, what + ": output, variant 6 vs 3")
    assert int(torch.unique(want).numel()) > 1000, "the GELU outputs barely vary: the comparison would see little"


# ---------------------------------------------------------------------------------------------------------------------
# (B) the automatic choice at its threshold


def _normal_bf16(shape, g, scale):
    """drawn directly in bf16: no f32 temporary of the operand's size"""
    t = torch.empty(shape, dtype=BF16, device=DEV)
    t.normal_(0.0, scale, generator=g)
    return t


def _written(p):
    return p.view(torch.int32) != SENT32


# (N, K, last M that runs variant 4, first M that runs variant 6, first plane row that tells)
THRESHOLD = [(2304, 768, 174720, 174721, 174592), (3072, 768, 130944, 130945, 130816), (768, 3072, 524160, 524161, 524032)]


@pytest.mark.parametrize("case", THRESHOLD, ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_automatic_choice_at_the_threshold(eng, case):
    N, K, m_lo, m_hi, tell = case
    assert m_hi == m_lo + 1 and -(-m_lo // TM) * (N // TN) < 16 * GRID <= -(-m_hi // TM) * (N // TN)  # the last M below, the first M at
    r3, r6 = m_hi // 256 * 256, m_hi // TM * TM
    assert (r3, r6) == (tell, tell + 128) and m_lo // 256 * 256 == r3  # the telling rows lie between the 256- and the 384-row interior
    g = _gen(4096 + N + K)
    A, W = _normal_bf16((m_hi, K), g, 1.0), _normal_bf16((N, K), g, 0.05)
    res = _normal_bf16((m_hi, N), g, 1.0)
    bias = _normal_bf16((N,), g, 0.5).float()
    what = f"variant 0, epilogue 8, N {N} K {K}"
    out3, p3, ran = launch(eng, 8, A, W, 3, bias=bias, res=res, planes=True, what=what + f" M {m_hi}, explicit variant 3")
    assert ran
    assert bool(_written(p3[:, :, :r3]).all()) and not bool(_written(p3[:, :, r3:]).any())
    # below: the 256-row kernel (variant 4)
    out, p, ran = launch(eng, 8, A[:m_lo], W, 0, bias=bias, res=res[:m_lo], planes=True, what=what + f" M {m_lo}")
    assert ran
    assert not bool(_written(p[:, :, r3:]).any()), f"{what} M {m_lo}: plane rows from {r3} on are written: the 384-row kernel ran below its threshold"
    assert bool(_written(p[:, :, :r3]).all())
    assert_bits(out.view(torch.int16), out3[:m_lo].view(torch.int16), what + f" M {m_lo}: output vs variant 3")
    del out, p
    # at: the 384-row kernel
    out, p, ran = launch(eng, 8, A, W, 0, bias=bias, res=res, planes=True, what=what + f" M {m_hi}")
    assert ran
    assert bool(_written(p[:, :, r3:r6]).all()), f"{what} M {m_hi}: plane rows {r3}..{r6 - 1} are not written: the 384-row kernel did not run at its threshold"
    assert bool(_written(p[:, :, :r3]).all()) and not bool(_written(p[:, :, r6:]).any())
    assert_bits(out.view(torch.int16), out3.view(torch.int16), what + f" M {m_hi}: output vs variant 3")
    assert_bits(p[:, :, :r3].contiguous().view(torch.int32).flatten(0, 1), p3[:, :, :r3].contiguous().view(torch.int32).flatten(0, 1),
                what + f" M {m_hi}: planes vs variant 3")


def test_automatic_choice_keeps_o_proj_on_the_256_row_kernel(eng):
    M, N, K = 524161, 768, 768
    r3, r6 = M // 256 * 256, M // TM * TM
    assert -(-M // TM) * (N // TN) >= 16 * GRID and r6 - r3 == 128
    g = _gen(4096 + N + K)
    A, W, res = _normal_bf16((M, K), g, 1.0), _normal_bf16((N, K), g, 0.05), _normal_bf16((M, N), g, 1.0)
    bias = _normal_bf16((N,), g, 0.5).float()
    what = f"variant 0, epilogue 8, M {M} N {N} K {K}"
    out, p, ran = launch(eng, 8, A, W, 0, bias=bias, res=res, planes=True, what=what)
    assert ran
    assert bool(_written(p[:, :, :r3]).all()) and not bool(_written(p[:, :, r3:]).any()), f"{what}: the planes are not those of 256-row interior tiles"
    out3, p3, _ = launch(eng, 8, A, W, 3, bias=bias, res=res, planes=True, what=what + ", explicit variant 3")
    assert_bits(out.view(torch.int16), out3.view(torch.int16), what + ": output vs variant 3")
    assert_bits(p.contiguous().view(torch.int32).flatten(0, 1), p3.contiguous().view(torch.int32).flatten(0, 1), what + ": planes vs variant 3")


# ---------------------------------------------------------------------------------------------------------------------
# (D) the product configuration end to end


def test_embed_above_the_thresholds_variant0_equals_variant4_in_bits():
    from multimodal_embeddings_amd import weights as Wt
    from multimodal_embeddings_amd._lib import Engine

    n, per = 2700, 224 * 224 * 3
    assert all(-(-n * 197 // TM) * (N // TN) >= 16 * GRID for N in (2304, 3072, 768))  # QKV, fc1, fc2 all take the 384-row kernel
    geom = dataclasses.replace(Wt.VIT_B16, num_layers=2)  # fc2 of the first block leaves the planes of the second block's LayerNorm
    e = Engine(0)
    try:
        e.load_vit(Wt.make_vit_weights(11, geom), geom=geom)
        e.set_chunk(n)
        pix = torch.zeros(n * per + 16, dtype=torch.uint8, device=DEV)
        pix[: n * per] = torch.randint(0, 256, (n * per,), generator=_gen(2700), device=DEV, dtype=torch.uint8)
        offs = np.arange(n, dtype=np.int64) * per
        hw = np.full((n, 2), 224, dtype=np.int32)
        ref = None
        for variant in (0, 4):
            e.set_gemm_variant(variant)
            for mode in (2, 1):
                e.set_ln_fusion(mode)
                got, _ = e.embed(pix, offs, hw)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(got).all()), (variant, mode)
                if ref is None:
                    ref = got.clone()
                assert torch.equal(ref.view(torch.int32), got.view(torch.int32)), f"gemm variant {variant}, ln fusion {mode}: embeddings differ in bits"
        assert int(torch.unique(ref[:, 0]).numel()) > n // 2, "the embeddings barely vary across crops"
    finally:
        e.close()
