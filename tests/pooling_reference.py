"""Test infrastructure of the mean-pooling tests (include/mme.h above mme_set_pooling): the covered grid
restated in Python, the pooled vectors over final-LayerNorm rows in a chosen dtype, and the mutants the tests must tell from
the definition.

    covered_grid(h, w, patch)          the fit-and-pad rule's (R, C): ceil(new_h / patch), ceil(new_w / patch)
    ln_rows(x, gamma, beta, eps, dt)   numpy LayerNorm of planted residual rows (the single-launch test)
    final_ln_rows(kind, ...)           the final-LayerNorm rows [n, T, D] of a seeded tower, through vit_hidden_states /
                                       dinov2_hidden_states and _final_ln of the existing reference modules
    pooled(y, grid, mode, mutant)      y [T, D] of one crop -> the "mean" vector [D] or the "cls+mean" vector [2 D]

Mutants: "whole_grid" (the mean over all g x g patches), "grid_transposed" ((C, R) for (R, C)), "row_short" (R - 1 rows, at
least one), "row_long" (R + 1, at most g), "cls_in_mean" (the class row joins the mean, divided by P + 1), "stride_g_plus_1"
(rows of the grid taken g + 1 tokens apart, indices capped at the last token), "divide_by_g2" (the sum divided by g * g
whatever P is: invisible under "mean", which normalises, and wrong under "cls+mean"), "l2_per_half" (cls+mean only: each half
normalised on its own).
"""
from __future__ import annotations

import math

import numpy as np
import torch

MUTANTS = ("whole_grid", "grid_transposed", "row_short", "row_long", "cls_in_mean", "stride_g_plus_1", "divide_by_g2", "l2_per_half")
CANVAS = 224


def fit_to_canvas(h: int, w: int):
    """(new_h, new_w) of the fit-and-pad rule (csrc/capi.hip, fit_to_canvas), the float expressions in its order"""
    scale_h, scale_w = CANVAS / h, CANVAS / w
    if scale_w < scale_h:
        return min(max(int(math.floor(h * scale_w)), 1), CANVAS), CANVAS
    return CANVAS, min(max(int(math.floor(w * scale_h)), 1), CANVAS)


def covered_grid(h: int, w: int, patch: int):
    nh, nw = fit_to_canvas(int(h), int(w))
    return -(-nh // patch), -(-nw // patch)


def ln_rows(x: np.ndarray, gamma: np.ndarray, beta: np.ndarray, eps: float, dtype) -> np.ndarray:
    """two-pass LayerNorm of the rows of x [..., d] in `dtype` (pool_ref of tests/test_gpu_gemm.py, without its L2 step)"""
    x, gamma, beta = x.astype(dtype), gamma.astype(dtype), beta.astype(dtype)
    mean = x.mean(-1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(eps)) * gamma + beta


@torch.no_grad()
def final_ln_rows(kind: str, pixel_values, w: dict, geom, dtype=torch.float64) -> np.ndarray:
    """[n, T, D]: every token row of a "vit" or "dinov2" tower behind its final LayerNorm, not normalised"""
    import dinov2_reference as dr
    import vit_reference as vr
    from clip_reference import layer_norm

    mod, hidden = (dr, dr.dinov2_hidden_states) if kind == "dinov2" else (vr, vr.vit_hidden_states)
    hs = hidden(pixel_values, w, geom, dtype)
    return layer_norm(hs, *mod._final_ln(w, dtype), geom.layer_norm_eps).numpy()


def l2(v: np.ndarray) -> np.ndarray:
    return v / np.maximum(np.sqrt((v * v).sum(dtype=v.dtype)), v.dtype.type(1e-12))


def pooled(y: np.ndarray, grid, mode: str, mutant: str | None = None) -> np.ndarray:
    """y [T, D] (T = 1 + g * g, row 0 the class row) -> the vector of `mode` ("mean" | "cls+mean") in y's dtype"""
    assert mode in ("mean", "cls+mean") and mutant in (None,) + MUTANTS
    T = y.shape[0]
    g = math.isqrt(T - 1)
    assert g * g == T - 1
    R, C = int(grid[0]), int(grid[1])
    assert 1 <= R <= g and 1 <= C <= g, (R, C, g)
    if mutant == "whole_grid":
        R, C = g, g
    elif mutant == "grid_transposed":
        R, C = C, R
    elif mutant == "row_short":
        R = max(R - 1, 1)
    elif mutant == "row_long":
        R = min(R + 1, g)
    stride = g + 1 if mutant == "stride_g_plus_1" else g
    idx = [min(1 + r * stride + c, T - 1) for r in range(R) for c in range(C)]
    if mutant == "cls_in_mean":
        idx = [0] + idx
    P = g * g if mutant == "divide_by_g2" else len(idx)
    m = y[idx].sum(0, dtype=y.dtype) / y.dtype.type(P)
    if mode == "mean":
        return l2(m)
    if mutant == "l2_per_half":
        return np.concatenate([l2(y[0]), l2(m)])
    return l2(np.concatenate([y[0], m]))


# ---- the inputs of the single-launch test (tests/test_gpu_pooling.py; tests/test_pooling_cpu.py measures the mutants on them) ----
SHAPES = ((197, 14), (50, 7), (257, 16))  # (tokens, g)
WIDTHS = (384, 768, 1024)
EPS = 1e-12


def planted_grids(g: int) -> np.ndarray:
    """nine grids, then those of the three special blocks (a row shifted by + 30, a row scaled x 100, a zero block)"""
    nine = [(g, g), (1, 1), (1, g), (g, 1), (5, g), (g, 5), (g - 1, g - 1), (2, 3), (min(10, g), min(14, g))]
    return np.array(nine + [(3, g), (g - 2, 4), (4, 4)], dtype=np.int32)


def planted(d: int, tokens: int, g: int):
    """-> x float32 [B, tokens, d] of bf16 values, gamma [d], beta [d] float32, grids int32 [B, 2]; B = 12"""
    grids = planted_grids(g)
    B = len(grids)
    rng = np.random.default_rng(1000 * d + tokens)
    x = rng.standard_normal((B, tokens, d)).astype(np.float32)
    x += rng.standard_normal((B, tokens, 1)).astype(np.float32)  # rows with means of their own
    x[9, 1 + g + 1] += 30.0   # inside the (3, g) grid
    x[10, 1 + 2] *= 100.0     # inside the (g - 2, 4) grid
    x[11] = 0.0               # every row LayerNorms to beta
    x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    gamma = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(d)).astype(np.float32)
    return x, gamma, beta, grids


def planted_reference(x, gamma, beta, grids, mode: str, dtype, mutant=None) -> np.ndarray:
    """[B, D] or [B, 2 D] in `dtype`: LayerNorm of every row, then pooled() per block"""
    y = ln_rows(x, gamma, beta, float(np.float32(EPS)), dtype)
    return np.stack([pooled(y[b], grids[b], mode, mutant) for b in range(len(grids))])


def one_minus_cos(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
