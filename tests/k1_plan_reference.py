"""K1's host plan restated in numpy, from the definitions and not from the planning code (csrc/k1_plan.h):

  * sizes: `oracle.preprocess.fit_to_canvas` (fit-and-pad), `optimal_tiled_canvas` / `fit_to_canvas_general` (tiles) and the
    transformers rule as tests/resize_spec_reference.py states it (specs), each vectorised over arrays of (h, w) in float64 with
    the operations in the scalar functions' order (tests/test_k1_plan_cpu.py holds the vectorised forms to the scalar ones);
  * windows: Pillow's Resample.c, precompute_coeffs -- ksize = 2 * ceil(support * max(in / out, 1)) + 1 in f64, support 1 for
    BILINEAR and 2 for BICUBIC; xmin = max(int(center - support' + 0.5), 0), xmax = min(int(center + support' + 0.5), in) with
    center = (xx + 0.5) * in / out and support' = support * max(in / out, 1);
  * the class of the horizontal pass: the rows of 3 * w bytes that fit beside the crop's table in the LDS budget, as
    `geometry_reference.h_pass_class` states it (whose text this module reuses for the fit-and-pad and tile tables).

`mutant` switches in one named mistake (MUTANTS); the CPU module asserts that its checks catch each on some size.
"""
from __future__ import annotations

import numpy as np

import geometry_reference as geo
from multimodal_embeddings_amd._lib import ResizeSpec

SIZE = 224
MAX_TAPS = 160
LDS_LIMIT = 160 * 1024
H_LDS_BUDGET = geo.H_LDS_BUDGET
SUPPORT = {2: 1.0, 3: 2.0}  # Pillow's resample number -> the filter's support
MUTANTS = ("ksize_without_plus_one", "class_budget_64k", "r0_from_top_plus_one")
# static LDS of the two vertical kernels beside their dynamic request: canvas 16 * 672 + 16, 16 windows, the 3 x 256 f32 table
V_STATIC_LDS = 16 * 672 + 16 + 16 * 8 + 3 * 256 * 4

# rule name -> ("fit_pad",) | ("spec", ResizeSpec) | ("tiles", tile, max_tiles); the specs: CLIP's, DINOv2's, ViT's, and the largest
# values mme_set_resize_spec admits (the smallest, 224, are CLIP's edge and ViT's exact size)
RULES = {
    "fit_pad": ("fit_pad",),
    "clip": ("spec", ResizeSpec("shortest_edge", 224, 0, 3)),
    "edge256_bicubic": ("spec", ResizeSpec("shortest_edge", 256, 0, 3)),
    "exact224_bilinear": ("spec", ResizeSpec("exact", 224, 224, 2)),
    "edge512_bicubic": ("spec", ResizeSpec("shortest_edge", 512, 0, 3)),
    "exact512_bicubic": ("spec", ResizeSpec("exact", 512, 512, 3)),
    "tiles560": ("tiles", 560, 4),
}


def engine_rule(rule):
    """(rule argument, keyword arguments) of Engine.k1_plan for a RULES value"""
    if rule[0] == "fit_pad":
        return "fit_pad", {}
    if rule[0] == "spec":
        return rule[1], {}
    return "tiles", {"tile": rule[1], "max_tiles": rule[2]}


def _floor_or_one(x):
    v = np.floor(x).astype(np.int64)
    return np.where(v == 0, 1, v)


def fit_sizes(h, w, target_h=SIZE, target_w=SIZE):
    """oracle.preprocess.fit_to_canvas / fit_to_canvas_general over arrays: (new_h, new_w)"""
    h = np.asarray(h, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    th = np.broadcast_to(np.asarray(target_h, dtype=np.int64), h.shape)
    tw = np.broadcast_to(np.asarray(target_w, dtype=np.int64), h.shape)
    scale_h, scale_w = th / h, tw / w
    by_w = scale_w < scale_h
    new_h = np.where(by_w, np.minimum(_floor_or_one(h * scale_w), th), th)
    new_w = np.where(by_w, tw, np.minimum(_floor_or_one(w * scale_h), tw))
    return new_h, new_w


def spec_sizes(spec: ResizeSpec, h, w):
    """resize_spec_reference.spec_geometry over arrays: (new_h, new_w, top, left)"""
    h = np.asarray(h, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    if spec.mode == "exact":
        new_h, new_w = np.full_like(h, spec.height), np.full_like(w, spec.width)
    else:
        short, long = np.minimum(h, w), np.maximum(h, w)
        new_long = ((spec.height * long).astype(np.float64) / short).astype(np.int64)  # int(size * long / short)
        new_h = np.where(h <= w, spec.height, new_long)
        new_w = np.where(h <= w, new_long, spec.height)
    return new_h, new_w, (new_h - SIZE) // 2, (new_w - SIZE) // 2


def tile_sizes(h, w, tile, max_tiles):
    """oracle.preprocess.optimal_tiled_canvas + fit_to_canvas_general over arrays: (th, tw, new_h, new_w)"""
    h = np.asarray(h, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    grids = [(a, b) for a in range(1, max_tiles + 1) for b in range(1, max_tiles + 1) if a * b <= max_tiles]
    ga = np.array([g[0] for g in grids], dtype=np.int64)[:, None]
    gb = np.array([g[1] for g in grids], dtype=np.int64)[:, None]
    scales = np.minimum((ga * tile) / h[None, :], (gb * tile) / w[None, :])  # [grids, n]
    up = scales >= 1
    sel = np.where(up.any(axis=0), np.where(up, scales, np.inf).min(axis=0), scales.max(axis=0))
    area = np.where(scales == sel[None, :], (ga * tile) * (gb * tile), np.iinfo(np.int64).max)
    pick = area.argmin(axis=0)  # the first of the smallest areas, in list order
    th, tw = ga[pick, 0], gb[pick, 0]
    target_w = np.minimum(np.maximum(w, tile), tw * tile)
    target_h = np.minimum(np.maximum(h, tile), th * tile)
    new_h, new_w = fit_sizes(h, w, target_h, target_w)
    return th, tw, new_h, new_w


def ksize(n_in, n_out, support=1.0, mutant=None):
    """Resample.c's ksize of an axis in f64"""
    n_in = np.asarray(n_in, dtype=np.float64)
    k = np.ceil(support * np.maximum(n_in / np.asarray(n_out, dtype=np.float64), 1.0)).astype(np.int64) * 2
    return k if mutant == "ksize_without_plus_one" else k + 1


def window(n_in, n_out, xx, support=1.0):
    """(xmin, xmax) of output coordinate xx: the first lines of precompute_coeffs"""
    n_in = np.asarray(n_in, dtype=np.int64)
    scale = n_in / np.asarray(n_out, dtype=np.float64)
    sup = support * np.maximum(scale, 1.0)
    center = (np.asarray(xx, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - sup + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + sup + 0.5).astype(np.int64), n_in)
    return xmin, xmax


def longest_window(n_in: int, n_out: int, first: int, count: int, support=1.0) -> int:
    """the true longest window among output coordinates [first, first + count) of one axis"""
    lo, hi = window(n_in, n_out, first + np.arange(count), support)
    return int((hi - lo).max())


def fit_rows(table, w, mutant=None):
    """rows of 3 * w bytes that fit beside a table of `table` bytes in the LDS budget (0 when the table alone does not fit)"""
    budget = 64 * 1024 if mutant == "class_budget_64k" else H_LDS_BUDGET
    return np.where(table < budget, (budget - table) // (3 * np.asarray(w, dtype=np.int64)), 0)


def pad(x, to):
    return -(-x // to) * to


def reference(rule, h, w, mutant=None) -> dict:
    """Every field of the plan the definitions fix, for arrays h, w under a RULES value.  Keys: new_h, new_w, top, left, th, tw,
    h_pass, v_pass, ksize_h, ksize_v (the f64 ksize of each filtered axis, 0 where not filtered), gh, kv (the capacities the table
    layouts round them up to), fit (rows beside the table), cls (-1 without bands), band_rows, n_bands, nrows (source rows the
    horizontal pass filters), tile_taps (tiles: the vertical window)."""
    h = np.asarray(h, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    R = {}
    sup = 1.0
    if rule[0] == "spec":
        spec = rule[1]
        sup = SUPPORT[spec.resample]
        R["new_h"], R["new_w"], R["top"], R["left"] = spec_sizes(spec, h, w)
        R["th"] = R["tw"] = np.ones_like(h)
    else:
        if rule[0] == "tiles":
            R["th"], R["tw"], R["new_h"], R["new_w"] = tile_sizes(h, w, rule[1], rule[2])
        else:
            R["new_h"], R["new_w"] = fit_sizes(h, w)
            R["th"] = R["tw"] = np.ones_like(h)
        R["top"] = R["left"] = np.zeros_like(h)
    hp, vp = R["new_w"] != w, R["new_h"] != h
    R["h_pass"], R["v_pass"] = hp, vp
    R["ksize_h"] = np.where(hp, ksize(w, R["new_w"], sup, mutant), 0)
    R["ksize_v"] = np.where(vp, ksize(h, R["new_h"], sup, mutant), 0)
    if rule[0] == "spec":
        # ClipLayout: an unfiltered axis holds one-tap windows (capacity one group / four taps); 224 columns always
        R["gh"] = (np.maximum(R["ksize_h"], 1) + 3) // 4
        R["kv"] = pad(np.maximum(R["ksize_v"], 1), 4)
        table = pad(SIZE * 8 + R["gh"] * SIZE * 16, 1024)
        top = R["top"] + (1 if mutant == "r0_from_top_plus_one" else 0)
        lo, _ = window(h, R["new_h"], top, sup)
        _, hi = window(h, R["new_h"], R["top"] + SIZE - 1, sup)
        R["r0"] = np.where(vp, lo, top)
        R["nr"] = np.where(vp, np.maximum(hi, lo + 1) - lo, SIZE)
        nrows = R["nr"]
        banded = np.ones_like(hp)
    else:
        R["gh"] = (R["ksize_h"] + 3) // 4
        R["kv"] = pad(R["ksize_v"], 4)
        table = pad(pad(R["new_w"] * 8, 16) + R["gh"] * R["new_w"] * 16, 1024)  # geometry_reference.h_pass_class's table
        R["r0"], R["nr"] = np.zeros_like(h), h
        nrows = h
        banded = hp
        R["tile_taps"] = np.where(vp, ksize(h, R["new_h"], 1.0), 1)
    fit = fit_rows(table, w, mutant)
    cls = np.where(fit >= 8, 0, np.where(fit >= 4, 1, 2))
    rows = np.where(cls == 0, np.minimum(fit // 8 * 8, 64), 4)
    R["table"] = table
    R["fit"] = np.where(banded, fit, -1)
    R["cls"] = np.where(banded, cls, -1)
    R["band_rows"] = np.where(banded, rows, 0)
    R["n_bands"] = np.where(banded, -(-nrows // np.maximum(rows, 1)), 0)
    R["nrows"] = np.where(banded, nrows, 0)
    # the dynamic LDS of the class's launch were this crop its widest: (table +) one band + 64 + the 1 KiB DMA slack
    band = np.minimum(rows, nrows) * 3 * w + np.where(cls < 2, table, 0)
    R["h_lds"] = np.where(banded, band + 64 + 1024, 0)
    return R


CLASS_NAMES = {0: "eight-row", 1: "four-row", 2: "through L1", -1: "none"}


def boundary_set(tile: int) -> np.ndarray:
    """1..300, every multiple of the tile up to 8000 with its two neighbours, and 7990..8000"""
    m = np.arange(tile, 8001, tile)
    s = np.concatenate([np.arange(1, 301), m - 1, m, m + 1, np.arange(7990, 8001)])
    return np.unique(s[(s >= 1) & (s <= 8000)])
