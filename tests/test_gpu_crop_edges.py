"""K0 (`crop_boxes`, csrc/preprocess.hip, through Engine.crop_boxes) on boxes at, over and far outside the edges of a page:
the zero fill, the bytes around the crops and the 64-bit box arithmetic.

Reference: `oracle.regions.crop_region` (PIL's Image.crop: the crop has the box's size, what lies outside the page is 0) on
the same seeded page; every byte of every crop is compared.  The pages (tests/geometry_reference.py) are 50 x 61 and 1 x 1
pixels with values 1..255, so a zero is always a fill and never a copy.

Cases, all boxes of a page in ONE call (geometry_reference.crop_cases): the whole page; one pixel at each corner; overhang
on each side and on the two sides of each corner; the page with a margin all round; boxes wholly outside on each side,
touching the edge (x0 == W, x1 == 0, ...) and one pixel away; 8000 x 1 and 1 x 8000 boxes through the page (one row per work
item / fewer rows than one item holds); a 131 x 400 box whose rows span five work items with the page's rows behind the
first; and the far-outside boxes x0 or y0 in {1431655766, 2^30, 2^31 - 11, -2^31, -2^30}, 10 wide and high, all zeros.
3 * 1431655766 = 2^32 + 2: a byte column formed in 32 bits lands on byte 2 of the page row.
Guards: `out` is pre-filled with 0xEE and the crops start at base = 4096; every byte outside the crops -- before `base`, the
alignment gaps between crops, the 16 bytes of slack and the rest of the buffer -- keeps 0xEE, and the page is unchanged.
Batch independence: each box gives the same crop when the list is reversed and when other boxes stand between.
Refusals: a box whose x1 - x0 or y1 - y0 does not fit 32 bits (-2^31 .. 2^31 - 1: 4294967295 wide, which wraps to -1) is
refused by index with its true size, by the binding and by the C entry point, like the other size errors; `out` is not
written and the next call works.

Mutants (asserted to differ from the oracle in tests/test_geometry_reference_cpu.py, each on a named case): clamp to the
edge instead of zero fill ("overhang right"); the right bound tested against W bytes instead of 3 W ("whole page"); 3 * x0
wrapped to 32 bits ("far x0=1431655766"); the row index taken without row0 ("several work items").

Measured on the MI355X: whole module 2.3 s, of which 2 s are the imports and the first engine; every case below 0.1 s
(each is one or two launches over at most 150 KB of crops).  On the commit before the fix the far box x0 = 1431655766 came
back with all of its 300 bytes copied from the page (1 of 30 on the 1 x 1 page); the other nine far boxes were zeros there
too, because their wrapped columns fall outside the row.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_reference as G  # noqa: E402
from oracle import regions as oreg  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
BASE = 4096


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


def _crop_all(engine, page_dev, boxes):
    """one call into a sentinel-filled buffer -> (host bytes of the whole buffer, offs, hw)"""
    offs_want, sizes, total = G.packed_layout(boxes, BASE)
    out = torch.full((BASE + total + 16 + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    pix, offs, hw = engine.crop_boxes(page_dev, boxes, out=out, base=BASE)
    torch.cuda.synchronize()
    assert pix is out and np.array_equal(offs, offs_want)
    assert np.array_equal(hw, np.asarray([(b[3] - b[1], b[2] - b[0]) for b in boxes], dtype=np.int32))
    return out.cpu().numpy(), offs, sizes


def _check(host, offs, sizes, page, cases):
    used = np.zeros(len(host), dtype=bool)
    bad = []
    for (case, box), o, s in zip(cases, offs, sizes):
        want = oreg.crop_region(page, box)
        got = host[o : o + s].reshape(want.shape)
        used[o : o + s] = True
        if not np.array_equal(got, want):
            bad.append((case, int((got != want).sum()), int(s)))
    assert not bad, f"(case, wrong bytes, bytes): {bad}"
    assert (host[~used] == SENTINEL).all(), "a byte outside the crops was written"
    assert not used[:BASE].any() and (~used).sum() >= BASE + 16 + 4096


@pytest.mark.parametrize("name", list(G.PAGES))
def test_every_byte_of_every_edge_crop_and_nothing_around_them(engine, name):
    page = G.page_pixels(name)
    page_dev = torch.from_numpy(page).cuda()
    cases = G.crop_cases(name)
    host, offs, sizes = _crop_all(engine, page_dev, [b for _, b in cases])
    _check(host, offs, sizes, page, cases)
    assert np.array_equal(page_dev.cpu().numpy(), page)


def test_far_outside_boxes_are_all_zeros(engine):
    """the predicted defect alone, so that its failure names it: 32-bit `x0 * 3` puts x0 = 1431655766 on byte 2 of the row"""
    page = G.page_pixels("50x61")
    cases = [c for c in G.crop_cases("50x61") if c[0].startswith("far")]
    assert len(cases) == 10
    host, offs, sizes = _crop_all(engine, torch.from_numpy(page).cuda(), [b for _, b in cases])
    nonzero = {case: int(np.count_nonzero(host[o : o + s])) for (case, _), o, s in zip(cases, offs, sizes)}
    print("non-zero bytes per far box:", nonzero)
    assert not any(nonzero.values()), nonzero


def test_crops_do_not_depend_on_their_neighbours(engine):
    page = G.page_pixels("50x61")
    page_dev = torch.from_numpy(page).cuda()
    cases = G.crop_cases("50x61")
    rev = cases[::-1]
    host, offs, sizes = _crop_all(engine, page_dev, [b for _, b in rev])
    _check(host, offs, sizes, page, rev)
    extra = [("extra", (k - 9, 3 * k - 20, k + 14, 3 * k + 1)) for k in range(len(cases))]
    mixed = [c for pair in zip(extra, cases) for c in pair]
    host, offs, sizes = _crop_all(engine, page_dev, [b for _, b in mixed])
    _check(host, offs, sizes, page, mixed)


def test_sizes_that_do_not_fit_are_refused_by_index_and_the_engine_goes_on(engine):
    from multimodal_embeddings_amd._lib import MmeError

    page = G.page_pixels("50x61")
    page_dev = torch.from_numpy(page).cuda()
    ok = (0, 0, 5, 5)
    lo, hi = -(2 ** 31), 2 ** 31 - 1
    for bad in [(lo, 0, hi, 5), (0, lo, 5, hi), (lo, 0, lo + 8001, 5), (hi, 0, lo, 5), (0, 0, 8001, 5)]:
        with pytest.raises(MmeError, match="box 1 is"):
            engine.crop_boxes(page_dev, [ok, bad])
    # the C entry point under the binding forms the same sizes in 64 bits and names the box too
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    offs = np.array([0, 80], dtype=np.int64)
    for bad, text in [((lo, 0, hi, 5), "box 1 is 4294967295x5"), ((0, hi, 5, lo), "box 1 is 5x-4294967295"), ((0, 0, 8001, 5), "box 1 is 8001x5")]:
        b = np.ascontiguousarray(np.array([ok, bad], dtype=np.int32))
        rc = engine.lib.mme_crop_boxes(engine.h, page_dev.data_ptr(), 50, 61, b.ctypes.data, 2, out.data_ptr(), offs.ctypes.data, engine._stream())
        assert rc != 0 and text in engine.lib.mme_last_error(engine.h).decode(), (bad, engine.lib.mme_last_error(engine.h).decode())
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    pix, offs, hw = engine.crop_boxes(page_dev, [(lo, 0, lo + 8000, 1), ok])
    host = pix.cpu().numpy()
    assert not host[: 8000 * 3].any() and np.array_equal(host[offs[1] : offs[1] + 75].reshape(5, 5, 3), page[:5, :5])
