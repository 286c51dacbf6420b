"""Planted inputs, switchable restatements and mutants for the three kernels between a detector's output and the encoder:
K0 (`crop_boxes`, cutting boxes out of a page), K13 (`nms_pages`, class-aware non-maximum suppression) and K1 tiles
(`resize_v_tiles`, the Mllama tile canvas).  Shared by tests/test_geometry_reference_cpu.py (no device) and
tests/test_gpu_crop_edges.py / test_gpu_nms_planted.py / test_gpu_tile_edges.py.

The REFERENCES are the oracle's: `oracle.regions.crop_region` (PIL's Image.crop), `oracle.regions.nms_keep`
(3_combine_grids.py:44-137) and `oracle.preprocess.preprocess_tiles` (image_processing_pil_mllama.py + Pillow's
Resample.c).  The restatements here (`crop_restated`, `nms_restated`, `tiles_restated`) are written from the same
definitions with one switch per named mistake; without a switch each must equal its oracle on every case (asserted in the
CPU module), with a switch it must differ on the case that names it.  Nothing here is taken from kernel code except the
sizes the cases aim at (32 KiB of box rows per work item, 256 lanes, 32768 boxes, 160 taps, the 32 KiB table budget).
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import preprocess as opre  # noqa: E402
from oracle import regions as oreg  # noqa: E402

# ======================================================================================================================
# K0: Image.crop of int boxes, zeros outside the page
# ======================================================================================================================

PAGES = {"50x61": (50, 61, 7), "1x1": (1, 1, 8)}  # name -> (H, W, seed)
WORK_ITEM_BYTES = 32 * 1024  # the rows of a box one work item of K0 cuts
FAR = (1431655766, 2 ** 30, 2 ** 31 - 11, -(2 ** 31), -(2 ** 30))  # 3 * 1431655766 = 2^32 + 2
CROP_MUTANTS = ("clamp_to_edge", "right_bound_w_bytes", "column_wraps_32_bits", "row_without_row0")
# the case of `crop_cases("50x61")` on which each mutant must differ
CROP_MUTANT_CASE = {"clamp_to_edge": "overhang right", "right_bound_w_bytes": "whole page", "column_wraps_32_bits": "far x0=1431655766",
                    "row_without_row0": "several work items"}


def page_pixels(name):
    """the seeded page, pixels 1..255: a zero in a crop is always a fill, never a copy"""
    H, W, seed = PAGES[name]
    return np.random.default_rng(seed).integers(1, 256, (H, W, 3), dtype=np.uint8)


def crop_cases(name):
    """[(case name, (x0, y0, x1, y1))] for a page, in the order of one device call"""
    H, W, _ = PAGES[name]
    c = [("whole page", (0, 0, W, H))]
    # one pixel at each corner
    c += [("corner tl", (0, 0, 1, 1)), ("corner tr", (W - 1, 0, W, 1)), ("corner bl", (0, H - 1, 1, H)), ("corner br", (W - 1, H - 1, W, H))]
    # overhang on one side, and on the two sides of each corner
    mx, my = W // 2, H // 2
    c += [("overhang left", (-7, my, mx + 1, my + 3)), ("overhang right", (mx, my, W + 9, my + 3)), ("overhang top", (mx, -5, mx + 4, my + 1)),
          ("overhang bottom", (mx, my, mx + 4, H + 6))]
    c += [("overhang tl", (-3, -4, 2, 2)), ("overhang tr", (W - 2, -4, W + 3, 2)), ("overhang bl", (-3, H - 2, 2, H + 4)), ("overhang br", (W - 2, H - 2, W + 3, H + 4))]
    c += [("margin all round", (-6, -5, W + 11, H + 9))]
    # wholly outside on each side: touching the edge, and one pixel away
    for d, tag in ((0, "touching"), (1, "one away")):
        c += [(f"outside right {tag}", (W + d, 0, W + d + 5, H)), (f"outside left {tag}", (-5 - d, 0, -d, H)),
              (f"outside below {tag}", (0, H + d, W, H + d + 4)), (f"outside above {tag}", (0, -4 - d, W, -d))]
    # one row per work item (24000 bytes a row) / fewer rows than one item holds (8000 rows of 3 bytes, 10922 fit)
    c += [("8000 wide, 1 high", (-4000 + mx, my, 4000 + mx, my + 1)), ("1 wide, 8000 high", (mx, -4000 + my, mx + 1, 4000 + my))]
    # rows of one box over several work items: (W + 70) * 3 bytes a row (393 on the 61-wide page: 83 rows an item), 400
    # rows; the page's rows start at row 170 of the box, behind the first item
    c += [("several work items", (-35, -170, W + 35, 230))]
    assert 170 >= WORK_ITEM_BYTES // ((W + 70) * 3) >= 1 and (W + 70) * 3 * 400 > WORK_ITEM_BYTES
    for v in FAR:
        c += [(f"far x0={v}", (v, 0, v + 10, min(H, 10))), (f"far y0={v}", (0, v, min(W, 10), v + 10))]
    return c


def crop_restated(page, box, mutant=None):
    """Image.crop((x0, y0, x1, y1)) on uint8[H, W, 3], byte by byte: byte b of row r of the crop is byte 3 * x0 + b of
    page row y0 + r where both exist, else 0.  `mutant` switches in one named mistake."""
    x0, y0, x1, y1 = (int(v) for v in box)
    H, W = page.shape[:2]
    h, w = y1 - y0, x1 - x0
    rows = page.reshape(H, W * 3)
    r = np.arange(h, dtype=np.int64)
    if mutant == "row_without_row0":  # every work item of the box starts again at the box's first row
        r = r % max(WORK_ITEM_BYTES // (w * 3), 1)
    y = y0 + r
    xb = 3 * x0 + np.arange(3 * w, dtype=np.int64)
    if mutant == "column_wraps_32_bits":
        xb = (xb + 2 ** 31) % 2 ** 32 - 2 ** 31
    if mutant == "clamp_to_edge":  # the edge pixel repeated instead of zeros
        px = np.clip(x0 + np.arange(w), 0, W - 1)
        return np.ascontiguousarray(page[np.clip(y, 0, H - 1)][:, px])
    ok_y = (y >= 0) & (y < H)
    ok_x = (xb >= 0) & (xb < (W if mutant == "right_bound_w_bytes" else 3 * W))
    out = np.zeros((h, 3 * w), dtype=np.uint8)
    if ok_y.any() and ok_x.any():
        out[np.ix_(ok_y, ok_x)] = rows[np.ix_(y[ok_y], xb[ok_x])]
    return out.reshape(h, w, 3)


def packed_layout(boxes, base=0):
    """(offs, sizes, total): crops 16-byte aligned from `base`, as Engine.crop_boxes documents its packing"""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    sizes = (b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0]) * 3
    offs = np.zeros(len(b), dtype=np.int64)
    if len(b) > 1:
        offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    return offs + base, sizes, int(offs[-1] + sizes[-1]) if len(b) else 0


# ======================================================================================================================
# K13: class-aware greedy non-maximum suppression
# ======================================================================================================================

NMS_MAX_BOXES = 32768
NMS_MUTANTS = ("greater_or_equal", "suppressed_boxes_suppress", "class_ignored", "last_of_equal_scores_first", "no_early_return",
               "union_without_inter", "bit_set_of_512_words")
# `touching_returns_early` (`<=` instead of `<` in the early return) is NOT in the list: it is an equivalent mutant.  Where
# xr == xl or yb == yt the area branch gives inter = +-0, so inter / union = +-0 if union > 0 and 0.0 otherwise -- the value
# the early return gives, and -0.0 compares like 0.0 against every threshold.  The CPU module asserts that equivalence on
# every planted page instead of a difference; `no_early_return` (disjoint boxes reach the area branch, where two negative
# extents multiply to a positive "intersection") is the detectable mistake about that branch.
NMS_EQUIVALENT_MUTANTS = ("touching_returns_early",)


def iou_restated(cur, others, mutant=None):
    """calculate_iou(box1 = the box just kept, box2), 3_combine_grids.py:44-78, float64 in its operation order"""
    cur = np.asarray(cur, dtype=np.float64)
    oth = np.asarray(others, dtype=np.float64).reshape(-1, 4)
    xl, yt = np.maximum(cur[0], oth[:, 0]), np.maximum(cur[1], oth[:, 1])
    xr, yb = np.minimum(cur[2], oth[:, 2]), np.minimum(cur[3], oth[:, 3])
    inter = (xr - xl) * (yb - yt)
    a1 = (cur[2] - cur[0]) * (cur[3] - cur[1])
    a2 = (oth[:, 2] - oth[:, 0]) * (oth[:, 3] - oth[:, 1])
    union = a1 + a2 if mutant == "union_without_inter" else (a1 + a2) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)
    if mutant == "no_early_return":
        return iou
    if mutant == "touching_returns_early":
        return np.where((xr <= xl) | (yb <= yt), 0.0, iou)
    return np.where((xr < xl) | (yb < yt), 0.0, iou)


def nms_restated(boxes, scores, classes, thr, mutant=None):
    """apply_non_max_suppression, 3_combine_grids.py:80-137: take the first of the highest scores that are left, keep it,
    drop every box left of its class whose IoU with it EXCEEDS the threshold; repeat.  Written as a walk over the stable
    descending-score order with a set of dropped boxes."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    classes = np.asarray(classes).reshape(-1)
    n = len(scores)
    tie = -1 if mutant == "last_of_equal_scores_first" else 1
    order = np.array(sorted(range(n), key=lambda i: (-scores[i], tie * i)), dtype=np.int64)
    bits = 512 * 32 if mutant == "bit_set_of_512_words" else max(n, 1)  # a short set: box j shares the bit of j - 16384
    dropped = np.zeros(bits, dtype=bool)
    keep = []
    for r, i in enumerate(order):
        if dropped[i % bits]:
            if mutant != "suppressed_boxes_suppress":
                continue
        else:
            keep.append(int(i))
        later = order[r + 1:]
        later = later[~dropped[later % bits]]
        if len(later):
            iou = iou_restated(boxes[i], boxes[later], mutant)
            hit = (iou >= thr) if mutant == "greater_or_equal" else (iou > thr)
            if mutant != "class_ignored":
                hit &= classes[later] == classes[i]
            dropped[later[hit] % bits] = True
    return keep


def _page(name, rule, boxes, scores, classes, thr, expect=None, mutants=()):
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    n = len(boxes)
    classes = np.asarray([classes] * n if np.isscalar(classes) else classes, dtype=np.int32)
    return {"name": name, "rule": rule, "boxes": boxes, "scores": np.asarray(scores, dtype=np.float64), "classes": classes, "thr": float(thr),
            "expect": expect, "mutants": tuple(mutants)}


def _tie_boxes(n, seed):
    """integer boxes on a 40 x 40 field, 4..12 wide: plenty of overlap above and below every threshold"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 40, (n, 2))
    return np.concatenate([xy, xy + rng.integers(4, 13, (n, 2))], axis=1).astype(np.float64)


def nms_planted_pages():
    """Every planted page with the rule that decides it.  `expect` is the kept list where the rule fixes it by hand (the
    oracle must agree); `mutants` are the switches that must change the kept list of THIS page."""
    P = []
    half = [[0, 0, 4, 4], [0, 0, 4, 2]]  # inter 8, union 16 + 8 - 8 = 16: IoU 0.5 exactly
    third = [[0, 0, 2, 2], [1, 0, 3, 2]]  # inter 2, union 4 + 4 - 2 = 6: IoU 2/6, the f64 quotient the threshold is computed as
    # IoU exactly on the threshold is NOT suppressed (`>`); one ulp lower it is
    P.append(_page("iou 1/2 at 1/2", "iou == threshold keeps both", half, [.9, .8], 0, 0.5, [0, 1], ["greater_or_equal"]))
    P.append(_page("iou 1/2 below 1/2", "iou > threshold drops the second", half, [.9, .8], 0, np.nextafter(0.5, 0), [0], ["union_without_inter"]))
    P.append(_page("iou 2/6 at 2/6", "iou == threshold keeps both", third, [.9, .8], 0, 2 / 6, [0, 1], ["greater_or_equal"]))
    P.append(_page("iou 2/6 below 2/6", "iou > threshold drops the second", third, [.9, .8], 0, np.nextafter(2 / 6, 0), [0], ["union_without_inter"]))
    # IoU(0,1) = IoU(1,2) = 60 / 140 > 0.4, IoU(0,2) = 20 / 180: the suppressed middle box must not suppress the third
    P.append(_page("greedy chain", "a suppressed box suppresses nothing", [[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]], [.9, .8, .7], 0, 0.4, [0, 2],
                   ["suppressed_boxes_suppress"]))
    # touching boxes (0, 1 share an edge; 0, 2 a corner) take the area branch: inter = 0, IoU 0.  Box 3 is disjoint from
    # box 0 on BOTH axes: without the early return (xr - xl) * (yb - yt) = (-1) * (-5) = 5 > 0 would count as overlap.
    # Box 4 has no area, box 5 is inverted (x1 < x0, y1 < y0; area +4 from two negative extents), box 6 is box 4 again:
    # union <= 0 -> IoU 0.  Nothing exceeds 0.0, so all are kept; at -0.1 the first box drops all of its class (0 > -0.1).
    touch = [[0, 0, 4, 4], [4, 0, 8, 4], [4, 4, 8, 8], [5, 9, 9, 13], [2, 2, 2, 2], [3, 3, 1, 1], [2, 2, 2, 2]]
    P.append(_page("touching and empty at 0", "IoU 0 never exceeds 0", touch, [.9, .8, .7, .6, .5, .4, .3], 0, 0.0, [0, 1, 2, 3, 4, 5, 6],
                   ["greater_or_equal", "no_early_return"]))
    P.append(_page("touching and empty below 0", "IoU 0 exceeds a negative threshold, also for disjoint boxes", touch, [.9, .8, .7, .6, .5, .4, .3],
                   [0, 0, 0, 0, 0, 1, 1], -0.1, [0, 5], ["class_ignored"]))
    # identical boxes: IoU 1 exceeds 0.95 but not 1.0
    same = [[1, 2, 9, 7]] * 4
    P.append(_page("identical at 0.95", "IoU 1 > 0.95", same, [.5, .9, .9, .1], 0, 0.95, [1]))
    P.append(_page("identical at 1", "IoU 1 is not > 1", same, [.5, .9, .9, .1], 0, 1.0, [1, 2, 0, 3], ["greater_or_equal", "last_of_equal_scores_first"]))
    # the same box in five classes, negative and large ids: classes never meet
    P.append(_page("five classes", "only the same class suppresses", [[0, 0, 5, 5]] * 5, [.1, .5, .3, .5, .2], [-2 ** 31, -1, 0, 7, 2 ** 31 - 1], 0.5,
                   [1, 3, 2, 4, 0], ["class_ignored"]))
    # ties: all scores equal -> the walk is in index order, over one stride of 256 lanes and more
    for n in (255, 256, 257, 1025):
        P.append(_page(f"all equal n={n}", "the first of equal scores goes first", _tie_boxes(n, n), np.full(n, 0.25), 0, 0.3, None,
                       ["last_of_equal_scores_first"] + (["suppressed_boxes_suppress", "greater_or_equal"] if n == 1025 else [])))
    # 0.0 == -0.0: index order decides; +-inf are ordered like any score
    pair = [[0, 0, 4, 4], [0, 0, 4, 3], [10, 0, 14, 4], [10, 0, 14, 3]]
    P.append(_page("signed zeros", "0.0 and -0.0 tie", pair, [-0.0, 0.0, 0.0, -0.0], 0, 0.5, [0, 2], ["last_of_equal_scores_first"]))
    P.append(_page("infinities", "+inf first, -inf last", pair + [[20, 0, 24, 4]], [-np.inf, np.inf, np.inf, 1e300, -np.inf], 0, 0.5, [1, 2, 4]))
    return P


def nms_scale_page():
    """32768 boxes of one class in 100 disjoint clusters (a 10 x 10 grid, 1000 apart) of boxes 100 +- 3 wide that are shifted
    by at most 3: IoU inside a cluster >= (97 / 106)^2 > 0.8, so about one box per cluster survives at 0.5.  The last box has
    the highest score of all: index 32767 is kept, and the other boxes of the last word of the bit set (32736..32766) are
    not."""
    rng = np.random.default_rng(32768)
    n = NMS_MAX_BOXES
    cl = rng.integers(0, 100, n)
    org = np.stack([cl % 10, cl // 10], axis=1) * 1000 + rng.integers(0, 4, (n, 2))
    boxes = np.concatenate([org, org + rng.integers(97, 104, (n, 2))], axis=1).astype(np.float64)
    scores = rng.integers(0, 4096, n) / 4096.0  # dyadic, with ties
    scores[n - 1] = 2.0
    return _page("32768 boxes", "the whole bit set of 1024 words", boxes, scores, 0, 0.5, None, ["bit_set_of_512_words"])


def nms_all_kept_page():
    """4096 disjoint boxes of one class on a 64 x 64 grid (9 wide, 10 apart): every box is kept, in score order"""
    rng = np.random.default_rng(4096)
    i = np.arange(4096)
    org = np.stack([i % 64, i // 64], axis=1) * 10
    boxes = np.concatenate([org, org + 9], axis=1).astype(np.float64)
    return _page("4096 kept", "4096 rounds of the walk", boxes, rng.permutation(4096) / 4096.0, 0, 0.5)


def nms_filler_pages(count=300, seed=13):
    """`count` random pages of 0..300 boxes on coordinates with one decimal, three classes; every fifth page empty"""
    rng = np.random.default_rng(seed)
    pages = []
    for p in range(count):
        n = 0 if p % 5 == 2 else int(rng.integers(0, 301))
        c = rng.uniform(0, 800, (n, 2))
        wh = rng.uniform(5, 300, (n, 2))
        boxes = np.round(np.concatenate([c - wh / 2, c + wh / 2], axis=1), 1)
        pages.append(_page(f"filler {p}", "", boxes, np.round(rng.uniform(0, 1, n), 2), rng.integers(0, 3, n).astype(np.int32), 0.5))
    return pages


def nms_batch(pages):
    """(boxes, scores, classes, page_offs) of a list of pages, for one call"""
    offs = np.zeros(len(pages) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(p["scores"]) for p in pages])
    return (np.concatenate([p["boxes"] for p in pages] + [np.zeros((0, 4))]), np.concatenate([p["scores"] for p in pages] + [np.zeros(0)]),
            np.concatenate([p["classes"] for p in pages] + [np.zeros(0, np.int32)]).astype(np.int32), offs)


def nms_oracle(page, thr=None):
    return oreg.nms_keep(page["boxes"], page["scores"], page["classes"], page["thr"] if thr is None else thr)


# ======================================================================================================================
# K1 tiles: the Mllama tile canvas
# ======================================================================================================================

MAX_TAPS = 160  # taps of one output row the vertical pass of the tile kernel holds
H_LDS_BUDGET = 32 * 1024  # LDS of one work item of the horizontal pass: table + rows
TILE_MUTANTS = ("padding_values_swapped", "vertical_taps_cut_at_160", "horizontal_taps_cut_at_160")

# (h, w) at tile 560 / 4 tiles, one mixed batch.  The comment is the horizontal-pass class (`h_pass_class`) and what is
# resized, as `tile_geometry` computes it (asserted in the CPU module).
SHAPES_560 = [
    (1, 1),        # eight-row; 560 x 560, both axes enlarged
    (1, 8000),     # through L1; 1 x 8000 -> 1 x 2240 in a 1 x 4 canvas, width only (the height stays 1)
    (8000, 1),     # none; 8000 x 1 -> 2240 x 1, height only
    (17, 8000),    # through L1; -> 4 x 2240
    (8000, 9),     # eight-row; -> 2240 x 2, a table of two columns
    (4000, 4000),  # through L1; -> 1120 x 1120 (the oracle takes 2.1 s for it; 8000 x 8000 is eight times the work)
    (560, 560),    # none; no pass at all
    (560, 1120),   # none; the 1 x 2 canvas met exactly
    (1120, 560),   # none; the 2 x 1 canvas met exactly
    (559, 2240),   # none; fits the 1 x 4 canvas one row short: nothing is resized, one row of padding
    (2240, 300),   # none; fits the 4 x 1 canvas: nothing is resized, 260 columns of padding
    (2800, 700),   # four-row; -> 2240 x 560: the table (22 KiB) leaves room for four rows of 2100 bytes, not eight
]
CLASS_560 = ["eight-row", "through L1", "none", "through L1", "eight-row", "through L1", "none", "none", "none", "none", "none", "four-row"]
OTHER_GEOMETRIES = [(16, 16), (64, 2), (224, 1), (336, 6), (1024, 1)]
OTHER_SHAPES = [(4000, 30), (30, 4000), (9, 8000), (1000, 999)]


def tile_image(h, w):
    return np.random.default_rng(h * 8191 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def tile_geometry(h, w, tile, max_tiles):
    """(tiles_h, tiles_w, new_h, new_w) from the oracle's canvas and fit rules"""
    ch, cw = opre.optimal_tiled_canvas(h, w, max_tiles, tile)
    new_h, new_w = opre.fit_to_canvas_general(h, w, ch, cw, tile)
    return ch // tile, cw // tile, new_h, new_w


def window_taps(in_size, out_size):
    """Resample.c's ksize of the triangle filter: the longest window of an axis, 1 if it is not resized"""
    return 1 if in_size == out_size else 2 * math.ceil(max(in_size / out_size, 1.0)) + 1


def h_pass_class(w, new_w):
    """The class of a crop's horizontal pass, restated from `k1_h_table_lds` and the 32 KiB budget: the table is a window
    (8 bytes) per output column padded to 16 bytes, plus 16 bytes per column and group of four taps, padded to 1 KiB; the
    rows of 3 * w bytes that fit beside it in 32 KiB decide: >= 8 eight-row items, >= 4 four-row items, else the table
    stays in memory and is read through L1."""
    if new_w == w:
        return "none"
    groups = (2 * -(-w // new_w) + 1 + 3) // 4
    table = -(-(-(-new_w * 8 // 16) * 16 + groups * new_w * 16) // 1024) * 1024
    fit = (H_LDS_BUDGET - table) // (3 * w) if table < H_LDS_BUDGET else 0
    return "eight-row" if fit >= 8 else "four-row" if fit >= 4 else "through L1"


def _coeffs(in_size, out_size, cap=None):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for the triangle filter as a dense [out, in] matrix of 22-bit
    weights; `cap` cuts every window to its first `cap` taps BEFORE the weights are normalised (the mutant)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    m = np.zeros((out_size, in_size), dtype=np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - fs + 0.5), 0)
        hi = min(int(center + fs + 0.5), in_size)
        if cap is not None:
            hi = min(hi, lo + cap)
        t = np.abs((np.arange(lo, hi, dtype=np.float64) - center + 0.5) * (1.0 / fs))
        wgt = np.where(t < 1.0, 1.0 - t, 0.0)
        ww = 0.0
        for v in wgt:
            ww += v
        if ww != 0.0:
            wgt = wgt / ww
        m[xx, lo:hi] = (0.5 + wgt * (1 << 22)).astype(np.int64)
    return m


def _pass(m, img):
    acc = (m @ img.reshape(img.shape[0], -1).astype(np.float64)).astype(np.int64) + (1 << 21)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8).reshape((m.shape[0],) + img.shape[1:])


def tiles_restated(img, tile, max_tiles, mutant=None):
    """image_processing_pil_mllama.py:483-541 -> f32 [max_tiles, 3, tile, tile]: resize into the canvas (horizontal pass,
    then vertical, each only if its size changes), pad with ZERO BYTES, normalise (so padding becomes lut[c][0]), split
    into tiles, unused tile slots +0.0."""
    h, w = img.shape[:2]
    th, tw, new_h, new_w = tile_geometry(h, w, tile, max_tiles)
    small = img
    if new_w != w:
        m = _coeffs(w, new_w, MAX_TAPS if mutant == "horizontal_taps_cut_at_160" else None)
        small = np.swapaxes(_pass(m, np.swapaxes(small, 0, 1)), 0, 1)
    if new_h != h:
        small = _pass(_coeffs(h, new_h, MAX_TAPS if mutant == "vertical_taps_cut_at_160" else None), small)
    lut = opre.normalise_lut()
    swapped = mutant == "padding_values_swapped"
    full = np.zeros((3, th * tile, tw * tile), dtype=np.float32)
    for c in range(3):
        full[c] = 0.0 if swapped else lut[c][0]
        full[c, :new_h, :new_w] = lut[c][small[:, :, c]]
    out = np.zeros((max_tiles, 3, tile, tile), dtype=np.float32)
    if swapped:
        out[:] = lut[:, 0][None, :, None, None]
    out[: th * tw] = full.reshape(3, th, tile, tw, tile).transpose(1, 3, 0, 2, 4).reshape(th * tw, 3, tile, tile)
    return out


def tallest_within_cap(tile):
    """the largest h whose vertical window at (tile, 1 tile) is still <= 160 taps when the height becomes `tile` rows, and
    h + 1, the smallest that exceeds it: 2 * ceil(h / tile) + 1 <= 160  <=>  ceil(h / tile) <= 79  <=>  h <= 79 * tile"""
    return 79 * tile, 79 * tile + 1
