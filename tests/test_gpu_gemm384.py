"""The 384 x 256 GEMM kernel (variant 6, csrc/gemm384r.hip) against the 256 x 256 kernel (variant 3), BIT FOR BIT.

Variant 6 runs the same MFMA with the same K order per accumulator and the same epilogue arithmetic as variant 3; only the
tile height, the LDS ring and the order in which a wave's row blocks are loaded and stored differ.  So every output element
and every LayerNorm partial-sum plane entry must be equal in bits, on random data (tests/test_gpu_gemm.py holds variant 3
against float64).  Each instantiated epilogue (0 bias, 1 GELU, 2 residual, 8 residual + planes, 5 folded LayerNorm,
6 folded LayerNorm + GELU) runs the smallest shapes at which the kernel takes another path:

  M = 384           one interior tile                      M = 896   two interior tiles and a ragged 128 rows
  M = 200           the edge path only                     M = 49 920, N = 512, K = 128   260 tiles on 256 workgroups: a
  N = 256, 320      full / ragged column tiles             workgroup runs a second tile (cross-tile ring, slot refill)
  K = 128, 192, 768 two, three and twelve K-tiles          reverse_m 0 and 1; the residual in place and out of place

Outputs sit between sentinel guard rows (Guard of tests/test_gpu_gemm.py).  Planes: both kernels leave them for the rows of
their own interior row tiles (256- and 384-row) and the column tiles that are whole; the rows both wrote must agree in bits,
and everything outside variant 6's interior must still hold the sentinel.  At M = 384 rows 256..383 are written by the
384-row kernel alone, which shows that it is the kernel that ran.

Last, a five-crop embed (985 token rows: two interior 384-row tiles and a ragged 217) under variants 3 and 6 with the
LayerNorm statistics from one pass over x (ln_fusion 1) and from the planes (ln_fusion 2): four embeddings equal in bits.

Everything beyond two tiles per workgroup is in tests/test_gpu_gemm384_stream.py: three and four tiles per workgroup, an odd
number of K-tiles across a tile boundary, several column groups, a ragged tile prefetched from an interior one and the
reverse, float64 exact references, the automatic choice (variant 0) at its threshold and the product configuration end to end.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_gemm import BF16, DEV, F32, SENT32, Guard, _gen, _randn, assert_bits  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


EPILOGUES = (0, 1, 2, 8, 5, 6)
# (M, N, K, reverse_m, residual in place)
SHAPES = [
    (384, 256, 128, 0, True),
    (896, 320, 192, 0, False),
    (896, 256, 768, 1, True),
    (200, 256, 768, 0, True),
    (49920, 512, 128, 0, True),
    (49920, 512, 128, 1, False),
]

_DATA = {}


def _data(M, N, K):
    """Operands of one shape, made once and shared by the epilogues (never modified: every launch writes its own Guard)."""
    key = (M, N, K)
    if key not in _DATA:
        g = _gen(384 + M + 7 * N + 13 * K)
        stats = torch.stack([_randn((M,), g, 0.1), 1.0 + _randn((M,), g, 0.1).abs()], dim=1).contiguous()
        _DATA[key] = dict(A=_randn((M, K), g, 1.0, BF16), W=_randn((N, K), g, 0.05, BF16), bias=_randn((N,), g, 0.5),
                          res=_randn((M, N), g, 1.0, BF16), stats=stats, colsum=_randn((N,), g, 0.5))
    return _DATA[key]


def _launch(eng, epi, d, variant, rev, inplace, what):
    M, N = d["A"].shape[0], d["W"].shape[0]
    out = Guard(BF16, M, N)
    kw = dict(variant=variant, reverse_m=rev, bias=d["bias"], out=out.view, ldo=out.ld)
    if epi in (2, 8):
        if inplace:
            out.valid.copy_(d["res"])
            kw["res"] = out.view
        else:
            rb = torch.zeros((M, out.ld), dtype=BF16, device=DEV)
            rb[:, :N] = d["res"]
            kw["res"] = rb
    if epi in (5, 6):
        kw.update(ln_stats=d["stats"], colsum=d["colsum"])
    planes = None
    if epi == 8:
        R = M + 5
        planes = Guard(F32, 1, 2 * (N // 64) * R, guard=64)
        kw.update(ln_part=planes.view, ln_part_rows=R)
    ran = eng.gemm_apply(epi, d["A"], d["W"], **kw)
    assert ran, f"{what}: a large-tile kernel must run"
    out.check(what)
    if planes is not None:
        planes.check(what + " (planes)")
        planes = planes.valid_bits().view(2, N // 64, -1)
    return out.valid_bits(), planes


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M{}-N{}-K{}-rev{}-{}".format(s[0], s[1], s[2], s[3], "inplace" if s[4] else "copy"))
def test_variant6_equals_variant3_in_bits(eng, epi, shape):
    M, N, K, rev, inplace = shape
    d = _data(M, N, K)
    what = f"epilogue {epi} M {M} N {N} K {K} reverse {rev}"
    want, pw = _launch(eng, epi, d, 3, rev, inplace, what + " variant 3")
    got, pg = _launch(eng, epi, d, 6, rev, inplace, what + " variant 6")
    assert_bits(got, want, what + ": output, variant 6 vs 3")
    if epi == 8:
        r3, r6, sl = M // 256 * 256, M // 384 * 384, N // 256 * 4  # interior rows of either kernel, slices of whole column tiles
        both = min(r3, r6)
        assert_bits(pg[:, :sl, :both], pw[:, :sl, :both], what + ": planes, variant 6 vs 3")
        assert bool((pg[:, :, r6:] == SENT32).all()) and bool((pg[:, sl:] == SENT32).all()), f"{what}: variant 6 wrote planes outside its interior tiles"
        if r6 > r3:  # rows only the 384-row kernel's interior tile covers
            assert bool((pg[:, :sl, r3:r6] != SENT32).all()), f"{what}: rows {r3}..{r6 - 1} of the planes were not written: the 384-row kernel did not run"


def test_embed_variant6_equals_variant3_in_bits():
    import numpy as np

    from multimodal_embeddings_amd._lib import Engine
    from multimodal_embeddings_amd.weights import make_vit_weights, synthetic_crops

    n = 5  # 985 token rows
    e = Engine(0)
    try:
        e.load_vit(make_vit_weights(seed=1))
        crops = synthetic_crops(n, seed=6)
        pix = torch.zeros(n * 224 * 224 * 3 + 16, dtype=torch.uint8, device=DEV)
        pix[: n * 224 * 224 * 3] = torch.from_numpy(crops.reshape(-1)).to(DEV)
        offs = np.arange(n, dtype=np.int64) * (224 * 224 * 3)
        hw = np.tile(np.array([[224, 224]], dtype=np.int32), (n, 1))
        ref = None
        for variant in (3, 6):
            e.set_gemm_variant(variant)
            for mode in (1, 2):
                e.set_ln_fusion(mode)
                got, _ = e.embed(pix, offs, hw)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(got).all()), (variant, mode)
                if ref is None:
                    ref = got.clone()
                assert torch.equal(ref.view(torch.int32), got.view(torch.int32)), f"gemm variant {variant}, ln fusion {mode}: embeddings differ in bits"
    finally:
        e.close()
