"""Float64 restatement of K17 (include/mme.h), numpy only: what the GPU tests compare with.

Moments: the rows are cut into blocks of BLOCK = MME_MOMENTS_BLOCK; inside a block every column sum and every product sum
starts from +0.0 and takes the rows in ascending order, one float64 addition per row (the product of two bf16 values has 16
significant bits and is exact in float64, so `acc + a * c` is the fused multiply-add of the kernel bit for bit); the blocks'
partials are added in ascending order on top of +0.0.  Projection: float64 from the same float32 mean and weights, with the
derived bound (d + 2) 2^-24 sum_c |x - mean| |w| beside it.
"""
from __future__ import annotations

import numpy as np

BLOCK = 1024  # MME_MOMENTS_BLOCK


def to_bf16_bits(x) -> np.ndarray:
    """float values -> the uint16 bit patterns of their bf16 roundings (nearest even; finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def bf16_bits_to_f64(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_exact(x) -> np.ndarray:
    """float values rounded to bf16, as float64"""
    return bf16_bits_to_f64(to_bf16_bits(x))


def moments(x64: np.ndarray, block: int = BLOCK, reverse: bool = False):
    """(sum [d], gram [d, d]) of the rows x64 [N, d] (float64 holding bf16 values) in the order of the definition.  `block` and
    `reverse` (the rows walked backwards) exist to show that the order matters (tests/test_projection_cpu.py)."""
    x = np.ascontiguousarray(x64, dtype=np.float64)
    if reverse:
        x = x[::-1]
    n, d = x.shape
    s, g = np.zeros(d), np.zeros((d, d))
    for b0 in range(0, n, block):
        ps, pg = np.zeros(d), np.zeros((d, d))
        for row in x[b0:b0 + block]:
            ps = ps + row
            pg = pg + np.multiply.outer(row, row)  # exact products, one addition each
        s = s + ps
        g = g + pg
    return s, g


def bits(a) -> np.ndarray:
    """float64 array -> its int64 bit patterns"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def project(x64: np.ndarray, mean32: np.ndarray, w32: np.ndarray):
    """(y64 [N, m], bound [N, m]): the projection in float64 from the float32 mean and weights, and the bound of mme.h on
    |y - y64| for an f32 kernel: one rounding for the difference, one for the product, at most d - 1 for the sum in any order."""
    mean32, w32 = np.asarray(mean32), np.asarray(w32)
    assert mean32.dtype == np.float32 and w32.dtype == np.float32
    c = np.asarray(x64, dtype=np.float64) - mean32.astype(np.float64)
    w = w32.astype(np.float64)
    d = c.shape[1]
    return c @ w.T, (d + 2) * 2.0 ** -24 * (np.abs(c) @ np.abs(w).T)


def normalise_rows(y32: np.ndarray) -> np.ndarray:
    """float64 unit rows of float32 coordinates (for comparisons with a tolerance; the bit-exact comparison is against the
    library's own row kernel)."""
    y = np.asarray(y32, dtype=np.float64)
    return y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)


def mixed_magnitudes(block: int = BLOCK, d: int = 64, seed: int = 1717, lo: int = -10, hi: int = 10) -> np.ndarray:
    """The fixture "mixed magnitudes": N = 3 block + 5 rows of bf16 values whose magnitudes span 2^lo .. 2^hi (2^-10 .. 2^10),
    both signs: the sums of their products round at almost every addition, so a different order of the rows or of the blocks
    changes bits of the gram.  (The column sums of 8-bit values over 20 binades are exact in any order; lo = -40, hi = 20 is
    the span at which they round too.)"""
    rng = np.random.default_rng(seed)
    n = 3 * block + 5
    x = rng.uniform(1.0, 2.0, (n, d)) * 2.0 ** rng.integers(lo, hi, (n, d)) * rng.choice([-1.0, 1.0], (n, d))
    return bf16_exact(x)


def planted(n: int, d: int, r: int, seed: int, noise: float = 0.01, mean_scale: float = 0.5):
    """Planted data for the fit: a mean, an orthonormal rank-r basis with variances 1, 1/2, 1/4, ..., isotropic noise.
    -> (x [n, d] float64, mean [d], basis [r, d], signal [n, d], noise [n, d])"""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((d, r)))[0].T
    mean = mean_scale * rng.standard_normal(d) / np.sqrt(d)
    sd = np.sqrt(0.5 ** np.arange(r))
    signal = (rng.standard_normal((n, r)) * sd) @ basis
    eps = noise * rng.standard_normal((n, d))
    return mean + signal + eps, mean, basis, signal, eps
