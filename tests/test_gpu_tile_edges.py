"""K1 tiles (`mme_preprocess_tiles`: the horizontal pass of csrc/resample.h and `resize_v_tiles`, csrc/preprocess.hip, through
Engine.preprocess_tiles) at the edges of what the API accepts: crops of 1 and 8000 pixels, canvases met exactly, tile sizes
8..1024, and the longest vertical window.

Reference: `oracle.preprocess.preprocess_tiles` (transformers image_processing_pil_mllama.py over Pillow's Resample.c).  The
f32 pixel values are compared as bit patterns, `aspect_ratio_id` and `num_tiles` exactly.  The output is pre-filled with
the NaN pattern 0x7FC0BEEF and has 4096 guard words before and behind it.

At tile 560 / 4 tiles, one mixed batch and the same batch reversed (h x w -> resized; class of the horizontal pass):
  1 x 1 -> 560 x 560, eight-row            1 x 8000 -> 1 x 2240, table through L1     8000 x 1 -> 2240 x 1, none
  17 x 8000 -> 4 x 2240, through L1        8000 x 9 -> 2240 x 2, eight-row            4000 x 4000 -> 1120 x 1120, through L1
  560 x 560, 560 x 1120, 1120 x 560: canvas met exactly, no pass at all
  559 x 2240 and 2240 x 300: the canvas' scale is >= 1 on both axes, nothing is resized; one row / 260 columns of padding
  2800 x 700 -> 2240 x 560, four-row (added here: no listed shape takes that class)
8000 x 8000 is left out: the oracle takes 2.1 s for 4000 x 4000 and would take eight times that.  The class rule, restated
from `k1_h_table_lds` and the 32 KiB budget (geometry_reference.h_pass_class): the table holds 8 bytes per output column
(padded to 16) plus 16 bytes per column and group of four taps, padded to 1 KiB; if eight source rows of 3 w bytes fit
beside it in 32 KiB the crop takes eight-row items, if four fit four-row items, else the table stays in memory and is read
through L1.  All three occur (asserted without a device).
Other geometries: (16, 16), (64, 2), (224, 1), (336, 6), (1024, 1) with crops 4000 x 30, 30 x 4000, 9 x 8000, 1000 x 999 --
vertical windows up to 127 taps, horizontal up to 127.  At (16, 1) the 9 x 8000 crop has a horizontal window of 1001 taps
and 30 x 4000 one of 501; that pass has no cap and is exact (4000 x 30 has a VERTICAL window of 501 taps there and stands
with the refused crops).
Padding: inside a used tile, canvas pixels outside the resized image are lut[c][0] (padding precedes normalisation);
unused tile slots are +0.0; nothing outside [n, max_tiles, 3, T, T] is written.
The long vertical window: the vertical pass holds 160 taps per output row.  8000 x 9 (1001 taps), 4000 x 30 (501) and
1265 x 9 (161) at (16, 1) and 633 x 9 at (8, 1) (161 taps, the smallest height there that exceeds the limit) are refused
with MME_E_ARG before any launch; the message names the crop, its size, the window and the limit; `out` keeps its pattern,
also where a valid crop stands before the refused one; the next call works.  632 x 9 at (8, 1) and 1264 x 9 at (16, 1) (159 taps: 2 * ceil(h / T) + 1 <= 160 <=> h <= 79 T) run
and are bit-exact.

Mutants (asserted to differ from the oracle in tests/test_geometry_reference_cpu.py): the two padding values swapped (on
every case with padding); the vertical taps cut at 160 (8000 x 9 at tile 16); the horizontal taps cut at 160 (9 x 8000).

Measured on the MI355X: whole module 3.5 s.  The 560 / 4 batch and its reverse take 1.0 s together (two device calls, the
oracle once for the twelve crops, 180 MB of output compared twice); (336, 6) and (1024, 1) 0.16 s each; every other case
below 0.05 s.  On the commit before the fix none of the four long-window batches was refused, and 4000 x 30 at (16, 1) came
back with 29 of its 48 resized values wrong.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_reference as G  # noqa: E402
from oracle import preprocess as opre  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF
GUARD = 4096


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


_reference = {}


def _want(h, w, tile, max_tiles):
    """the oracle's output for a seeded crop, computed once and left unchanged"""
    key = (h, w, tile, max_tiles)
    if key not in _reference:
        out, aid, nt, _ = opre.preprocess_tiles(G.tile_image(h, w), tile, max_tiles)
        out.setflags(write=False)
        _reference[key] = (out, aid, nt)
    return _reference[key]


def _pack(shapes):
    arrays = [G.tile_image(h, w) for h, w in shapes]
    hw = np.array(shapes, dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(shapes), dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).cuda(), offs, hw


def _sentinel_out(n, tile, max_tiles):
    words = n * max_tiles * 3 * tile * tile
    flat = torch.full((words + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return flat, flat[GUARD : GUARD + words].view(n, max_tiles, 3, tile, tile)


def _run_and_check(engine, shapes, tile, max_tiles):
    pix, offs, hw = _pack(shapes)
    flat, out = _sentinel_out(len(shapes), tile, max_tiles)
    pv, ids, mask, nt = engine.preprocess_tiles(pix, offs, hw, tile, max_tiles, out=out)
    torch.cuda.synchronize()
    assert pv is out
    bits = flat.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == NAN_BITS).all() and (bits[-GUARD:] == NAN_BITS).all(), "written outside [n, max_tiles, 3, T, T]"
    host = bits[GUARD:-GUARD].reshape(len(shapes), max_tiles, 3, tile, tile)
    lut = opre.normalise_lut().view(np.uint32)
    bad = []
    for k, (h, w) in enumerate(shapes):
        want, aid, n_t = _want(h, w, tile, max_tiles)
        if int(ids[k]) != aid or nt[k] != n_t or mask[k].tolist() != [1] * n_t + [0] * (max_tiles - n_t):
            bad.append(((h, w), "grid", int(ids[k]), nt[k]))
        elif not np.array_equal(host[k], want.view(np.uint32)):
            bad.append(((h, w), "pixels", int((host[k] != want.view(np.uint32)).sum())))
        # the padding rules, stated on their own
        th, tw, new_h, new_w = G.tile_geometry(h, w, tile, max_tiles)
        assert not host[k, th * tw :].any(), ((h, w), "an unused tile slot is not +0.0")
        canvas = host[k, : th * tw].reshape(th, tw, 3, tile, tile).transpose(2, 0, 3, 1, 4).reshape(3, th * tile, tw * tile)
        for c in range(3):
            assert (canvas[c, new_h:, :] == lut[c, 0]).all() and (canvas[c, :, new_w:] == lut[c, 0]).all(), ((h, w), "padding is not lut[c][0]")
    assert not bad, (tile, max_tiles, bad)


def test_tile_560_mixed_batch_and_reversed(engine):
    assert [G.h_pass_class(w, G.tile_geometry(h, w, 560, 4)[3]) for h, w in G.SHAPES_560] == G.CLASS_560
    assert {"eight-row", "four-row", "through L1"} <= set(G.CLASS_560)
    _run_and_check(engine, G.SHAPES_560, 560, 4)
    _run_and_check(engine, G.SHAPES_560[::-1], 560, 4)


@pytest.mark.parametrize("tile,max_tiles", G.OTHER_GEOMETRIES)
def test_other_tile_geometries(engine, tile, max_tiles):
    _run_and_check(engine, G.OTHER_SHAPES, tile, max_tiles)


def test_a_horizontal_window_of_1001_taps_is_exact(engine):
    """(16, 1): 9 x 8000 -> 1 x 16.  The horizontal table is sized from the crop, so no window is too long for it.  (4000 x 30
    of the other geometries' crops has a VERTICAL window of 501 taps here and stands with the refused ones below.)"""
    shapes = [(9, 8000), (30, 4000), (1000, 999)]
    assert [G.window_taps(w, G.tile_geometry(h, w, 16, 1)[3]) for h, w in shapes] == [1001, 501, 135]
    _run_and_check(engine, shapes, 16, 1)


def test_the_window_at_the_limit_is_exact(engine):
    for tile in (8, 16):
        ok, _ = G.tallest_within_cap(tile)
        assert G.window_taps(ok, tile) == 159
        _run_and_check(engine, [(40, 33), (ok, 9), (ok - 1, 9), (ok, 40)], tile, 1)


@pytest.mark.parametrize("tile,shape,taps", [(16, (8000, 9), 1001), (8, (633, 9), 161), (16, (1265, 9), 161), (16, (4000, 30), 501)])
def test_a_longer_vertical_window_is_refused_before_any_launch(engine, tile, shape, taps):
    from multimodal_embeddings_amd._lib import MmeError

    assert G.window_taps(shape[0], G.tile_geometry(*shape, tile, 1)[2]) == taps > G.MAX_TAPS
    shapes = [(40, 33), shape, (20, 20)]  # a valid crop before and behind: the batch is refused whole
    pix, offs, hw = _pack(shapes)
    flat, out = _sentinel_out(3, tile, 1)
    with pytest.raises(MmeError) as e:
        engine.preprocess_tiles(pix, offs, hw, tile, 1, out=out)
    text = str(e.value)
    assert "(-1)" in text and "crop 1 " in text and f"{shape[0]}x{shape[1]}" in text and f"{taps} taps" in text and "160 taps" in text, text
    torch.cuda.synchronize()
    assert (flat.view(torch.int32) == NAN_BITS).all(), "the refused call wrote to `out`"
    _run_and_check(engine, [(40, 33), (20, 20)], tile, 1)  # the next call on the context works
