"""The planted inputs of tests/geometry_reference.py without a GPU: that each switchable restatement equals its oracle where
no switch is set, that the hand-written expectations are the oracle's, that no case is vacuous, and that every named
mutant is visible on the case that names it -- known to hold before anything reaches a GPU.

K0: `crop_restated` == oracle.regions.crop_region on every box of both pages (and == PIL's Image.crop wherever PIL takes
the box); the far-outside boxes are all zeros in the oracle; mutants clamp_to_edge, right_bound_w_bytes,
column_wraps_32_bits, row_without_row0 each differ on CROP_MUTANT_CASE.
K13: `nms_restated` == oracle.regions.nms_keep on every planted page, the 32768-box page, the 4096-box page and filler
pages; the seven NMS_MUTANTS each change the kept list of the pages that name them, and every mutant is named.
`touching_returns_early` is an EQUIVALENT mutant (geometry_reference.NMS_EQUIVALENT_MUTANTS says why): it is asserted to
change nothing on any planted page, so that nobody takes it for covered.
K1 tiles: `tiles_restated` == oracle.preprocess.preprocess_tiles on small crops at four geometries; the class of every
560 / 4 shape is the listed one and all three classes occur; padding_values_swapped differs wherever there is padding;
the taps cut at 160 differ on 8000 x 9 (vertical) and 9 x 8000 (horizontal) at tile 16: the first is why such a crop is
refused, the second why the horizontal pass must have no cap.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_reference as G  # noqa: E402
from oracle import preprocess as opre  # noqa: E402
from oracle import regions as oreg  # noqa: E402


# ---- K0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.PAGES))
def test_crop_restatement_equals_the_oracle_and_pil(name):
    from PIL import Image

    page = G.page_pixels(name)
    assert page.min() >= 1
    img = Image.fromarray(page)
    H, W = page.shape[:2]
    for case, box in G.crop_cases(name):
        want = oreg.crop_region(page, box)
        assert want.shape == (box[3] - box[1], box[2] - box[0], 3), case
        assert np.array_equal(G.crop_restated(page, box), want), case
        if not case.startswith("far"):
            assert np.array_equal(np.array(img.crop(box)), want), case
        inside = want[max(-box[1], 0) : max(min(box[3], H) - box[1], 0), max(-box[0], 0) : max(min(box[2], W) - box[0], 0)]
        assert (inside != 0).all() and int((want != 0).sum()) == inside.size, case  # zeros are exactly the fill
        if case.startswith(("far", "outside")):
            assert not want.any(), case
    names = [c for c, _ in G.crop_cases(name)]
    assert len(set(names)) == len(names) and len([c for c in names if c.startswith("far")]) == 10


@pytest.mark.parametrize("mutant", G.CROP_MUTANTS)
def test_crop_mutants_differ_on_their_case(mutant):
    page = G.page_pixels("50x61")
    box = dict(G.crop_cases("50x61"))[G.CROP_MUTANT_CASE[mutant]]
    assert not np.array_equal(G.crop_restated(page, box, mutant), oreg.crop_region(page, box))


def test_the_wrapped_column_of_the_far_box_lands_inside_the_page():
    assert 3 * 1431655766 - 2 ** 32 == 2
    page = G.page_pixels("50x61")
    got = G.crop_restated(page, (1431655766, 0, 1431655776, 10), "column_wraps_32_bits")
    assert np.array_equal(got.reshape(10, 30), page.reshape(50, 183)[:10, 2:32])  # page bytes where the crop has zeros
    for v in G.FAR[1:]:  # the other far corners wrap to columns outside the page: they guard the fix, not the defect
        assert not G.crop_restated(page, (v, 0, v + 10, 10), "column_wraps_32_bits").any()


# ---- K13 ---------------------------------------------------------------------------------------------------------------
def test_nms_planted_pages_are_the_oracles_and_their_mutants_show():
    named = set()
    for p in G.nms_planted_pages():
        want = G.nms_oracle(p)
        if p["expect"] is not None:
            assert want == p["expect"], p["name"]
        assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"]) == want, p["name"]
        for m in p["mutants"]:
            assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"], m) != want, (p["name"], m)
            named.add(m)
        for m in G.NMS_EQUIVALENT_MUTANTS:
            assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"], m) == want, (p["name"], m)
        if p["name"].startswith("all equal"):
            assert want == sorted(want) and 3 < len(want) < len(p["scores"]) // 2, p["name"]
    assert named | {"bit_set_of_512_words"} == set(G.NMS_MUTANTS)


def test_nms_thresholds_are_the_planted_ious():
    half, third = [p for p in G.nms_planted_pages() if p["name"] in ("iou 1/2 at 1/2", "iou 2/6 at 2/6")]
    assert oreg.box_iou(half["boxes"][0], half["boxes"][1:])[0] == 0.5 == half["thr"]
    assert oreg.box_iou(third["boxes"][0], third["boxes"][1:])[0] == 2 / 6 == third["thr"]
    chain = next(p for p in G.nms_planted_pages() if p["name"] == "greedy chain")
    b = chain["boxes"]
    assert oreg.box_iou(b[0], b[1:]).tolist() == [60 / 140, 20 / 180] and oreg.box_iou(b[1], b[2:])[0] == 60 / 140


def test_nms_scale_pages_use_the_whole_bit_set():
    p = G.nms_scale_page()
    n = len(p["scores"])
    assert n == G.NMS_MAX_BOXES == 32768
    want = G.nms_oracle(p)
    assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"]) == want
    last_word = [i for i in want if i >= n - 32]
    print(f"32768 boxes: {len(want)} kept, of the last word {last_word}")
    assert 90 <= len(want) <= 130 and want[0] == n - 1 and last_word == [n - 1]  # 31 of the last word's 32 are suppressed
    assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"], "bit_set_of_512_words") != want
    q = G.nms_all_kept_page()
    want = G.nms_oracle(q)
    assert sorted(want) == list(range(4096)) and want == np.argsort(-q["scores"], kind="stable").tolist()
    assert G.nms_restated(q["boxes"], q["scores"], q["classes"], q["thr"]) == want


def test_nms_filler_pages_are_mixed():
    pages = G.nms_filler_pages()
    sizes = [len(p["scores"]) for p in pages]
    assert len(pages) == 300 and sizes.count(0) >= 60 and max(sizes) > 280 and sizes[2] == 0
    for p in pages[:12]:
        want = G.nms_oracle(p)
        assert G.nms_restated(p["boxes"], p["scores"], p["classes"], p["thr"]) == want
        assert len(want) < len(p["scores"]) or len(want) < 5


# ---- K1 tiles ----------------------------------------------------------------------------------------------------------
SMALL_TILE_CASES = [((16, 16), (17, 90)), ((16, 16), (100, 99)), ((64, 2), (300, 17)), ((224, 1), (40, 33)), ((8, 1), (8, 8)), ((16, 1), (1264, 9))]


@pytest.mark.parametrize("geometry,shape", SMALL_TILE_CASES)
def test_tiles_restatement_equals_the_oracle_and_swapped_padding_shows(geometry, shape):
    tile, max_tiles = geometry
    img = G.tile_image(*shape)
    want = opre.preprocess_tiles(img, tile, max_tiles)[0]
    assert np.array_equal(G.tiles_restated(img, tile, max_tiles).view(np.uint32), want.view(np.uint32))
    th, tw, new_h, new_w = G.tile_geometry(*shape, tile, max_tiles)
    has_padding = th * tw < max_tiles or new_h < th * tile or new_w < tw * tile
    differs = not np.array_equal(G.tiles_restated(img, tile, max_tiles, "padding_values_swapped"), want)
    assert differs == has_padding, (geometry, shape)
    for m in ("vertical_taps_cut_at_160", "horizontal_taps_cut_at_160"):  # windows within the cap: the cut changes nothing
        assert np.array_equal(G.tiles_restated(img, tile, max_tiles, m), want)


def test_tile_shapes_take_the_listed_classes_and_all_three_occur():
    got = []
    for h, w in G.SHAPES_560:
        _, _, new_h, new_w = G.tile_geometry(h, w, 560, 4)
        got.append(G.h_pass_class(w, new_w))
        assert G.window_taps(h, new_h) <= 17  # far below the cap at the model's geometry
    assert got == G.CLASS_560
    assert {"eight-row", "four-row", "through L1", "none"} == set(got)
    for tile, mt in G.OTHER_GEOMETRIES:
        for h, w in G.OTHER_SHAPES:
            _, _, new_h, _ = G.tile_geometry(h, w, tile, mt)
            assert G.window_taps(h, new_h) <= G.MAX_TAPS, (tile, mt, h, w)  # every listed case is inside the limit and must run
    assert G.window_taps(8000, G.tile_geometry(9, 8000, 16, 1)[3]) == 1001  # the horizontal window that has no cap


def test_the_cut_taps_are_wrong_pixels_and_the_limit_heights_are_exact():
    tall, wide = G.tile_image(8000, 9), G.tile_image(9, 8000)
    want = opre.preprocess_tiles(tall, 16, 1)[0]
    assert G.tile_geometry(8000, 9, 16, 1)[2:] == (16, 1) and G.window_taps(8000, 16) == 1001
    assert np.array_equal(G.tiles_restated(tall, 16, 1), want)
    assert not np.array_equal(G.tiles_restated(tall, 16, 1, "vertical_taps_cut_at_160"), want)
    want = opre.preprocess_tiles(wide, 16, 1)[0]
    assert np.array_equal(G.tiles_restated(wide, 16, 1), want)
    assert not np.array_equal(G.tiles_restated(wide, 16, 1, "horizontal_taps_cut_at_160"), want)
    for tile in (8, 16):
        ok, over = G.tallest_within_cap(tile)
        assert G.tile_geometry(ok, 9, tile, 1)[2] == tile == G.tile_geometry(over, 9, tile, 1)[2]
        assert G.window_taps(ok, tile) == 159 <= G.MAX_TAPS < 161 == G.window_taps(over, tile)
        assert G.window_taps(ok - 1, tile) == 159 and over <= 8000
    assert G.tallest_within_cap(8) == (632, 633) and G.tallest_within_cap(16) == (1264, 1265)
