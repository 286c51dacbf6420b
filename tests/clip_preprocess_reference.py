"""CLIP's own preprocessing restated in numpy: shortest-edge BICUBIC resize to 224, centre crop 224 x 224.

What `CLIPImageProcessorPil` (transformers 5.15.0) does to one uint8 HWC image before rescale / normalise:
  * image_transforms.get_resize_output_image_size, `size = {"shortest_edge": 224}`, default_to_square = False:
    the short edge becomes 224, the long edge int(224 * long / short)                              -> `clip_resize_geometry`
  * image_processing_backends.PilBackend.resize -> Pillow `Image.resize((new_w, new_h), BICUBIC)`  -> `clip_window_u8`
  * image_processing_backends.PilBackend.center_crop to 224 x 224: top = (new_h - 224) // 2, left = (new_w - 224) // 2

Pillow 12.2 libImaging/Resample.c, 8 bits per channel: separable, horizontal pass then vertical pass, an axis whose size
does not change is not filtered; bicubic filter with a = -0.5 and support 2 (times the down-scale factor); coefficients
normalised in f64, quantised to 22 fractional bits with ties away from zero; each pass adds 2^21, shifts right by 22
(arithmetic) and clamps to 0..255.

Only the 224 x 224 window of the resized image is computed: an output coordinate's taps depend on (in_size, out_size,
coordinate) alone, so the resized image (1.8 million pixels long for a 1 x 8000 crop) never exists.  The horizontal pass
runs over the source rows the vertical windows touch and nothing else.

tests/test_clip_preprocess_cpu.py pins this file against Pillow and transformers (live where they import, and through the
hashes of tests/golden/clip_preprocess_cases.json everywhere).
"""
from __future__ import annotations

import math

import numpy as np

SIZE = 224
PRECISION_BITS = 32 - 8 - 2  # Resample.c


def clip_resize_geometry(h: int, w: int, size: int = SIZE) -> tuple[int, int, int, int]:
    """(new_h, new_w, top, left): the resized size and the centre-crop origin of an h x w image."""
    short, long = (h, w) if h <= w else (w, h)
    new_short, new_long = size, int(size * long / short)  # Python float: size * long first, then the division
    new_h, new_w = (new_short, new_long) if h <= w else (new_long, new_short)
    return new_h, new_w, (new_h - size) // 2, (new_w - size) // 2


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_taps(in_size: int, out_size: int, first: int, count: int):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for output coordinates [first, first + count) of the full
    axis: (xmin[count], n[count], kk[count, ksize] int64)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin = np.zeros(count, dtype=np.int64)
    cnt = np.zeros(count, dtype=np.int64)
    kk = np.zeros((count, ksize), dtype=np.int64)
    for i in range(count):
        center = (first + i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = [_bicubic((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:  # summed sequentially, as Resample.c does
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[i], cnt[i] = lo, n
        kk[i, :n] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, cnt, kk


def _apply(m: np.ndarray, src: np.ndarray) -> np.ndarray:
    """clip8((2^21 + m @ src) >> 22) along axis 0; exact in f64: |sum| < 255 * 1.25 * 2^22 + 2^21 < 2^31."""
    shp = src.shape
    acc = m @ src.reshape(shp[0], -1).astype(np.float64)
    acc = acc.astype(np.int64) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8).reshape((m.shape[0],) + shp[1:])


def _window_matrix(in_size: int, out_size: int, first: int, count: int):
    """(m f64 [count, hi - lo], lo, hi): the fixed-point taps of outputs [first, first + count) over source [lo, hi)."""
    xmin, cnt, kk = bicubic_taps(in_size, out_size, first, count)
    lo, hi = int(xmin.min()), int((xmin + cnt).max())
    m = np.zeros((count, hi - lo), dtype=np.float64)
    for i in range(count):
        m[i, xmin[i] - lo : xmin[i] - lo + cnt[i]] = kk[i, : cnt[i]]
    return m, lo, hi


def clip_window_u8(img: np.ndarray, size: int = SIZE) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [224, 224, 3]: `Image.resize((new_w, new_h), BICUBIC)` then the centre crop, bit for bit."""
    h, w = img.shape[:2]
    new_h, new_w, top, left = clip_resize_geometry(h, w, size)
    # the source rows the vertical windows touch (all `size` rows from `top` when the height does not change)
    if new_h != h:
        mv, r0, r1 = _window_matrix(h, new_h, top, size)
    else:
        mv, r0, r1 = None, top, top + size
    rows = img[r0:r1]
    if new_w != w:
        mh, c0, c1 = _window_matrix(w, new_w, left, size)
        rows = np.swapaxes(_apply(mh, np.swapaxes(rows[:, c0:c1], 0, 1)), 0, 1)
    else:
        rows = rows[:, left : left + size]
    if mv is not None:
        rows = _apply(mv, rows)
    return np.ascontiguousarray(rows)


def tap_ranges(h: int, w: int, size: int = SIZE) -> dict:
    """Largest |coefficient|, largest sum of |coefficients| and most taps over both axes' windows of an h x w crop."""
    new_h, new_w, top, left = clip_resize_geometry(h, w, size)
    out = {"max_coeff": 0, "max_abs_sum": 0, "max_taps": 0}
    for n_in, n_out, first in ((w, new_w, left), (h, new_h, top)):
        if n_in == n_out:
            continue
        _, cnt, kk = bicubic_taps(n_in, n_out, first, size)
        out["max_coeff"] = max(out["max_coeff"], int(np.abs(kk).max()))
        out["max_abs_sum"] = max(out["max_abs_sum"], int(np.abs(kk).sum(axis=1).max()))
        out["max_taps"] = max(out["max_taps"], int(cnt.max()))
    return out


# ---- the test cases shared by the CPU and GPU tests and by tests/golden/make_clip_preprocess_golden.py ----------------
SHAPES = [(224, 224), (224, 300), (300, 224), (225, 224), (224, 225), (449, 448), (112, 112), (5, 7), (1, 1), (1, 9), (300, 500), (640, 480),
          (2000, 3000), (37, 1000), (1000, 37), (17, 224), (223, 900), (600, 1400)]
BIG_SHAPE = (8000, 7168)  # the 143-tap case and the size limit: noise only


def case_list():
    """[(name, kind, h, w, seed)]: every shape as seeded noise and as a seeded 0/255 image, the big shape as noise only."""
    cases = []
    for i, (h, w) in enumerate(SHAPES):
        cases.append((f"noise_{h}x{w}", "noise", h, w, 1000 + i))
        cases.append((f"binary_{h}x{w}", "binary", h, w, 2000 + i))
    cases.append((f"noise_{BIG_SHAPE[0]}x{BIG_SHAPE[1]}", "noise", BIG_SHAPE[0], BIG_SHAPE[1], 3000))
    return cases


def case_image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "binary":  # drives the negative lobes into both clamps
        return (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    raise ValueError(kind)


def bundled_crop(golden_dir: str, name: str) -> np.ndarray:
    from PIL import Image

    import os

    return np.asarray(Image.open(os.path.join(golden_dir, "crops", name)).convert("RGB"))


_windows: dict = {}


def restated_window(key, img: np.ndarray) -> np.ndarray:
    """clip_window_u8(img), computed once per `key` and shared by the tests of a session (read-only)."""
    if key not in _windows:
        w = clip_window_u8(img)
        w.setflags(write=False)
        _windows[key] = w
    return _windows[key]
