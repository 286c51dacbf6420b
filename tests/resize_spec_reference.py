"""A checkpoint's own preprocessing restated in numpy: resize the whole image as a `ResizeSpec` says, centre crop 224 x 224.

What the Pillow backends of transformers' image processors (5.15.0: ViTImageProcessorPil, SiglipImageProcessorPil,
BitImageProcessorPil, CLIPImageProcessorPil) do to one uint8 HWC image before rescale / normalise:
  * the resized size: `size = {"height", "width"}` is taken as it is, the aspect not kept; `size = {"shortest_edge": S}` is
    image_transforms.get_resize_output_image_size: the short edge S, the long edge int(S * long / short)  -> `spec_geometry`
  * image_processing_backends.PilBackend.resize -> Pillow `Image.resize((new_w, new_h), resample)`         -> `spec_window_u8`
  * PilBackend.center_crop to 224 x 224: top = (new_h - 224) // 2, left = (new_w - 224) // 2 (absent for an exact 224 target,
    whose window has the origin (0, 0))

This is tests/clip_preprocess_reference.py over (resized size, window origin, filter): the same Resample.c arithmetic (its
`_apply`, its bicubic filter, its 22-bit rounding) with the triangle filter beside the bicubic one.  Only the 224 x 224 window
of the resized image is computed.  tests/test_resize_spec_cpu.py pins this file against Pillow and transformers (live where
they import, and through the hashes of tests/golden/resize_spec_cases.json everywhere).
"""
from __future__ import annotations

import math

import numpy as np

import clip_preprocess_reference as cpr
from multimodal_embeddings_amd._lib import ResizeSpec

SIZE = cpr.SIZE
PRECISION_BITS = cpr.PRECISION_BITS


def _triangle(x: float) -> float:  # Resample.c bilinear_filter
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {2: (_triangle, 1.0), 3: (cpr._bicubic, 2.0)}  # Pillow's resample number -> (filter, support)


def spec_geometry(spec: ResizeSpec, h: int, w: int) -> tuple[int, int, int, int]:
    """(new_h, new_w, top, left): the resized size and the centre-crop origin of an h x w image under `spec`."""
    if spec.mode == "exact":
        new_h, new_w = spec.height, spec.width
    else:
        new_h, new_w = cpr.clip_resize_geometry(h, w, spec.height)[:2]
    return new_h, new_w, (new_h - SIZE) // 2, (new_w - SIZE) // 2


def filter_taps(resample: int, in_size: int, out_size: int, first: int, count: int):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for output coordinates [first, first + count) of the full
    axis under Pillow's filter `resample`: (xmin[count], n[count], kk[count, ksize] int64)."""
    filt, sup = FILTERS[resample]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = sup * filterscale
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
        w = [filt((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:  # summed sequentially, as Resample.c does
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[i], cnt[i] = lo, n
        kk[i, :n] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return xmin, cnt, kk


def _window_matrix(resample: int, in_size: int, out_size: int, first: int, count: int):
    """(m f64 [count, hi - lo], lo, hi): the fixed-point taps of outputs [first, first + count) over source [lo, hi)."""
    xmin, cnt, kk = filter_taps(resample, in_size, out_size, first, count)
    lo, hi = int(xmin.min()), int((xmin + cnt).max())
    m = np.zeros((count, hi - lo), dtype=np.float64)
    for i in range(count):
        m[i, xmin[i] - lo : xmin[i] - lo + cnt[i]] = kk[i, : cnt[i]]
    return m, lo, hi


def spec_window_u8(spec: ResizeSpec, img: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [224, 224, 3]: `Image.resize((new_w, new_h), spec.resample)` then the centre crop, bit for
    bit.  Horizontal pass over the source rows the vertical windows touch, then the vertical pass; an axis whose size does
    not change is not filtered.  (`cpr._apply` is exact in f64: 255 * sum |k| + 2^21 < 2^31 << 2^53.)"""
    h, w = img.shape[:2]
    new_h, new_w, top, left = spec_geometry(spec, h, w)
    if new_h != h:
        mv, r0, r1 = _window_matrix(spec.resample, h, new_h, top, SIZE)
    else:
        mv, r0, r1 = None, top, top + SIZE
    rows = img[r0:r1]
    if new_w != w:
        mh, c0, c1 = _window_matrix(spec.resample, w, new_w, left, SIZE)
        rows = np.swapaxes(cpr._apply(mh, np.swapaxes(rows[:, c0:c1], 0, 1)), 0, 1)
    else:
        rows = rows[:, left : left + SIZE]
    if mv is not None:
        rows = cpr._apply(mv, rows)
    return np.ascontiguousarray(rows)


def tap_ranges(spec: ResizeSpec, h: int, w: int) -> dict:
    """Largest |coefficient|, largest sum of |coefficients| and most taps over both axes' windows of an h x w crop."""
    new_h, new_w, top, left = spec_geometry(spec, h, w)
    out = {"max_coeff": 0, "max_abs_sum": 0, "max_taps": 0}
    for n_in, n_out, first in ((w, new_w, left), (h, new_h, top)):
        if n_in == n_out:
            continue
        _, cnt, kk = filter_taps(spec.resample, n_in, n_out, first, SIZE)
        out["max_coeff"] = max(out["max_coeff"], int(np.abs(kk).max()))
        out["max_abs_sum"] = max(out["max_abs_sum"], int(np.abs(kk).sum(axis=1).max()))
        out["max_taps"] = max(out["max_taps"], int(cnt.max()))
    return out


# ---- the cases shared by the CPU and GPU tests and by tests/golden/make_resize_spec_golden.py ---------------------------
SPECS = {
    "exact224_bicubic": ResizeSpec("exact", 224, 224, 3),          # SiglipImageProcessor
    "exact224_bilinear": ResizeSpec("exact", 224, 224, 2),         # ViTImageProcessor; SigLIP 2 directories with resample 2
    "edge256_bicubic": ResizeSpec("shortest_edge", 256, 0, 3),     # BitImageProcessor as DINOv2 directories configure it
    "exact256_bicubic": ResizeSpec("exact", 256, 256, 3),          # DeiT-style: 256 x 256, then the 224 x 224 centre
}
SHAPES = [(1, 1), (1, 9), (5, 7), (17, 224), (112, 112), (224, 224), (224, 225), (225, 224), (224, 300), (300, 224), (255, 256), (256, 256),
          (257, 256), (256, 300), (223, 900), (37, 1000), (1000, 37), (640, 480), (3000, 230), (8000, 224), (224, 8000)]


def case_list():
    """[(name, kind, h, w, seed)]: every shape as seeded noise and as a seeded 0/255 image."""
    cases = []
    for i, (h, w) in enumerate(SHAPES):
        cases.append((f"noise_{h}x{w}", "noise", h, w, 5000 + i))
        cases.append((f"binary_{h}x{w}", "binary", h, w, 6000 + i))
    return cases


_images: dict = {}
_windows: dict = {}


def case_image(name: str, kind: str, h: int, w: int, seed: int) -> np.ndarray:
    """The case's image, made once per session (read-only)."""
    if name not in _images:
        a = cpr.case_image(kind, h, w, seed)
        a.setflags(write=False)
        _images[name] = a
    return _images[name]


def restated_window(spec_key: str, name, img: np.ndarray) -> np.ndarray:
    """spec_window_u8(SPECS[spec_key], img), computed once per (spec, name) and shared by the tests of a session (read-only)."""
    key = (spec_key, name)
    if key not in _windows:
        win = spec_window_u8(SPECS[spec_key], img)
        win.setflags(write=False)
        _windows[key] = win
    return _windows[key]
