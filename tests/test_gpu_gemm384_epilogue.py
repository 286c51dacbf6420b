"""The folded-LayerNorm epilogues (5, 6) of the 384 x 256 GEMM kernel (variant 6) on PLANTED operands, against exact values.

The kernel fetches a tile's bias, column sums and row statistics under its K loop, one value per lane, and hands every lane
its own columns 16 j + 4 fq + r and rows 16 i + fr by cross-lane moves in the epilogue.  What can go wrong there is a lane
map (a row or column block taken from another lane) or a tile that computes with the operands of the tile before it.
The bit tests against variant 3 (tests/test_gpu_gemm384.py, tests/test_gpu_gemm384_stream.py) would see either on random
data; this file pins both on values that name the row and column they belong to, against a table and not another kernel:

  A = 0 (every accumulator is exactly +0), W random,
  mean[m] = (m mod 251) - 125    rstd[m] = 2^((m mod 5) - 2)    colsum[n] = (n mod 127) - 63    bias[n] = 0.25 (n mod 61)

Every product and sum of rstd * (-mean * colsum) + bias is exact in f32 (|mean * colsum| <= 7875, rstd a power of two,
bias a multiple of 1/4 below 16: multiples of 1/16 below 2^15), so epilogue 5 must give bf16_rne of the float64 table
IN BITS.  Epilogue 6 puts the erf-GELU (a fit with no exact float64 twin) on the same values and is held to variant 3 in
bits on the same operands.

The plant is only worth something if a wrong map changes the table: test_plant_tells_the_mutants (CPU) builds the five
tables a wrong kernel would give -- statistics of row m + 16; bias and colsum of column n + 4; of column n + 16; the
statistics of the row panel before (m - 384); the bias of the column tile before (n - 256) -- and requires each to differ
from the expected table in at least half of its elements (bf16 bits), on every shape class below.

Shapes (variant 6 forced, reverse_m 0 and 1 each):
  (384, 256, 128)       one interior tile, two K-tiles: K-tile 0 is the one that fetches the operands
  (896, 320, 192)       ragged rows and columns beside interior tiles (the guarded path loads for itself)
  (49 920, 320, 128)    260 tiles on 256 workgroups: a workgroup's second tile lies in another column tile
  (50 120, 512, 128)    a ragged row tile; with reverse_m = 1 it comes first and an interior tile follows it in the workgroup
  (147 840, 512, 192)   three tiles per workgroup, three K-tiles
At N = 320 the second column tile is ragged: its tiles take the guarded path, which loads its own operands.  So the two
N = 320 shapes show that a guarded tile is not disturbed by (and does not disturb) the operands its interior neighbours
fetched early, but a change of column tile BETWEEN two early fetches of one workgroup happens in the N = 512 shapes only.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_gemm import BF16, DEV, F32, F64, Guard, _gen, _randn, assert_bits  # noqa: E402

SHAPES = [(384, 256, 128), (896, 320, 192), (49920, 320, 128), (50120, 512, 128), (147840, 512, 192)]
TM, TN = 384, 256  # the kernel's tile


def plant(M, N, dev, row_shift=0, col_shift=0, bias_shift=0):
    """-> mean [M], rstd [M], colsum [N], bias [N] in float64; the shifts give the operands a mutant kernel would use."""
    m = torch.arange(M, device=dev) + row_shift
    n = torch.arange(N, device=dev)
    mean = ((m % 251) - 125).to(F64)
    rstd = torch.pow(2.0, ((m % 5) - 2).to(F64))
    colsum = (((n + col_shift) % 127) - 63).to(F64)
    bias = 0.25 * ((n + bias_shift) % 61).to(F64)
    return mean, rstd, colsum, bias


def table_bits(M, N, dev, **shifts):
    """bf16 bits of rstd * (-mean * colsum) + bias, from float64; asserts that f32 holds every value exactly."""
    mean, rstd, colsum, bias = plant(M, N, dev, **shifts)
    v = rstd[:, None] * (-mean[:, None] * colsum[None, :]) + bias[None, :]
    v32 = v.float()
    assert torch.equal(v32.double(), v), "the planted table is not exact in f32"
    return v32.to(BF16).view(torch.int16)


MUTANTS = {
    "rows shifted by 16": dict(row_shift=16),
    "columns shifted by 4": dict(col_shift=4, bias_shift=4),
    "columns shifted by 16": dict(col_shift=16, bias_shift=16),
    "statistics of the previous row panel": dict(row_shift=-TM),
    "bias of the previous column tile": dict(bias_shift=-TN),
}


@pytest.mark.parametrize("shape", [(384, 256), (896, 320), (2510, 320), (2510, 512)], ids=lambda s: f"M{s[0]}-N{s[1]}")
def test_plant_tells_the_mutants(shape):
    """CPU.  Rows repeat with period lcm(251, 5) = 1255: 2510 rows stand for the long shapes."""
    M, N = shape
    want = table_bits(M, N, "cpu")
    for name, shifts in MUTANTS.items():
        differ = int((table_bits(M, N, "cpu", **shifts) != want).sum())
        print(f"M {M} N {N} mutant '{name}': {differ} of {want.numel()} elements differ")
        assert 2 * differ >= want.numel(), f"mutant '{name}' differs from the expected table in {differ} of {want.numel()} elements only"


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()
    _DATA.clear()


_DATA = {}


def _data(M, N, K):
    """Operands and the expected bits of one shape, made once (never modified: every launch writes its own Guard)."""
    key = (M, N, K)
    if key not in _DATA:
        mean, rstd, colsum, bias = plant(M, N, DEV)
        _DATA[key] = dict(A=torch.zeros((M, K), dtype=BF16, device=DEV), W=_randn((N, K), _gen(5 + M + N + K), 0.05, BF16),
                          stats=torch.stack([mean, rstd], dim=1).to(F32).contiguous(), colsum=colsum.to(F32), bias=bias.to(F32),
                          want=table_bits(M, N, DEV))
    return _DATA[key]


def _launch(eng, epi, d, variant, rev, what):
    M, N = d["A"].shape[0], d["W"].shape[0]
    out = Guard(BF16, M, N)
    ran = eng.gemm_apply(epi, d["A"], d["W"], variant=variant, reverse_m=rev, bias=d["bias"], out=out.view, ldo=out.ld, ln_stats=d["stats"],
                         colsum=d["colsum"])
    assert ran, f"{what}: a large-tile kernel must run"
    out.check(what)
    return out.valid_bits()


@pytest.mark.gpu
@pytest.mark.parametrize("rev", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M{}-N{}-K{}".format(*s))
def test_epilogue5_equals_the_planted_table_in_bits(eng, shape, rev):
    M, N, K = shape
    d = _data(M, N, K)
    what = f"epilogue 5 M {M} N {N} K {K} reverse {rev} variant 6"
    assert_bits(_launch(eng, 5, d, 6, rev, what), d["want"], what + " vs the planted table")


@pytest.mark.gpu
@pytest.mark.parametrize("rev", (0, 1))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M{}-N{}-K{}".format(*s))
def test_epilogue6_equals_variant3_in_bits(eng, shape, rev):
    M, N, K = shape
    d = _data(M, N, K)
    what = f"epilogue 6 M {M} N {N} K {K} reverse {rev}"
    want = _launch(eng, 6, d, 3, rev, what + " variant 3")
    assert_bits(_launch(eng, 6, d, 6, rev, what + " variant 6"), want, what + ": variant 6 vs 3")
