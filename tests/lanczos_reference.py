"""numpy restatement of `Image.resize((new_w, new_h), Image.LANCZOS)` for 8-bit RGB (Pillow libImaging/Resample.c, 8-bit
path), the reference of tests/test_lanczos_cpu.py and tests/test_gpu_lanczos.py.

Filter: lanczos(x) = sinc(x) sinc(x / 3) on -3 <= x < 3, sinc(0) = 1, else sin(pi x) / (pi x); support 3.
Per axis (precompute_coeffs, box = whole image): scale = in / out, filterscale = max(scale, 1), support = 3 * filterscale,
ksize = 2 * ceil(support) + 1; per output coordinate center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
xmax = min(int(center + support + 0.5), in); weights lanczos((x + xmin - center + 0.5) * (1 / filterscale)) summed
sequentially into ww and divided by it; fixed point (int)(+-0.5 + w * 2^22).  Horizontal pass, then vertical pass, each a
signed 32-bit sum from 2^21, shifted arithmetically by 22, clamped to 0..255.  An axis whose size does not change is not
filtered.  One exception to the order, made in PIL/Image.py (Pillow 12): an image more than 100 times as high as wide that
gets lower is resized vertically first (`vertical_first`).

The weights are evaluated one by one with math.sin (libm's sin, the function Pillow's object code calls): numpy's
vectorised sin is another implementation and may differ in the last bit, which can flip a fixed-point rounding.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
CAP = 8000  # config.MAX_IMAGE_HEIGHT_AND_WIDTH


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def ksize_of(in_size: int, out_size: int) -> int:
    scale = in_size / out_size
    return int(math.ceil(3.0 * max(scale, 1.0))) * 2 + 1


def tables(in_size: int, out_size: int):
    """-> (bounds int32[out, 2] {xmin, n}, coeffs int32[out, ksize]) of one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coeffs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return bounds, coeffs


def _pass(img: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """One integer pass along axis 0: img uint8 [in, ...] -> uint8 [out, ...]."""
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        k = coeffs[xx, :n].astype(np.int64)
        acc = np.tensordot(k, src[xmin : xmin + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2**31  # the 32-bit accumulator of Resample.c does not overflow
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_with_tables(img: np.ndarray, new_h: int, new_w: int, tables_fn=tables) -> np.ndarray:
    """The two integer passes over tables from `tables_fn(in, out)`; img uint8 [h, w, 3] -> uint8 [new_h, new_w, 3]."""
    h, w = img.shape[:2]
    if new_h < 1 or new_w < 1:
        raise ValueError("height and width must be > 0")
    a = img

    def horizontal(a):
        return a if new_w == w else np.swapaxes(_pass(np.swapaxes(a, 0, 1), *tables_fn(w, new_w)), 0, 1)

    def vertical(a):
        return a if new_h == h else _pass(a, *tables_fn(h, new_h))

    if vertical_first(h, w, new_h):
        a = horizontal(vertical(a))
    else:
        a = vertical(horizontal(a))
    return np.ascontiguousarray(a)


def vertical_first(h: int, w: int, new_h: int) -> bool:
    """Image.resize (PIL/Image.py) shrinks a very tall image vertically first, as two calls of the C resize:
    `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`.  Every other image: horizontal pass, then vertical.
    The intermediate image is rounded to bytes either way, so the order shows in the result."""
    return h > w * 100 and new_h < h


def resize(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    return resize_with_tables(img, new_h, new_w)


def capped_size(h: int, w: int):
    """(new_h, new_w) of embedder.py:110-114 for an image with a side over CAP: the reference's own expression."""
    scale = CAP / max(w, h)
    return int(h * scale), int(w * scale)


def make_image(seed: int, h: int, w: int, kind: str) -> np.ndarray:
    """The seeded test images: "noise" = uniform bytes, "binary" = 0 / 255 only (the negative lobes hit both clamps)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    raise ValueError(kind)
