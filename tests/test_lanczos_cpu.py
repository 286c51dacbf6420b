"""The device cap's host side, without a GPU: the numpy restatement of Pillow's LANCZOS resize against live Pillow, the
library's tables (mme_lanczos_tables) through the restatement's integer passes, the coefficient bounds the kernels rely on,
the size rule of embedder.py:110-114, and the argument refusals of the entries that need no device.  Every comparison of
pixels is bit equality."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import lanczos_reference as ref  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "lanczos_cases.json")))
CASES = GOLDEN["cases"]
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def lib():
    from multimodal_embeddings_amd.build import build
    from multimodal_embeddings_amd._lib import load_library

    return load_library(build())


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pillow(img, nh, nw):
    from PIL import Image

    return np.asarray(Image.fromarray(img).resize((nw, nh), Image.LANCZOS))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_pillow(case):
    """(a) tests/lanczos_reference.py == Image.resize(..., LANCZOS), byte for byte, and the recorded hashes are Pillow's."""
    import PIL

    for kind in ("noise", "binary"):
        img = ref.make_image(case["seed"], case["h"], case["w"], kind)
        got = ref.resize(img, case["new_h"], case["new_w"])
        want = _pillow(img, case["new_h"], case["new_w"])
        assert got.shape == want.shape and np.array_equal(got, want), (case["name"], kind, int((got != want).sum()))
        if PIL.__version__ == GOLDEN["pillow"]:
            assert _sha(want) == case["sha256"][kind]
        if kind == "binary" and case["name"] in ("gen_upscale", "cap_300x8001", "cap_9000x10", "tile_at"):
            # the negative lobes drive sums below 0 and above 255: both clamps are met (not just reached by plain 0 / 255 runs)
            f = ref.resize(img.astype(np.int64).clip(0, 1).astype(np.uint8) * 128, case["new_h"], case["new_w"])
            assert want.min() == 0 and want.max() == 255 and f.max() > 128 and f.min() == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_library_tables_reproduce_pillow(lib, case):
    """(b) the restatement's two integer passes over the tables mme_lanczos_tables returns give Pillow's bytes, and the
    tables themselves equal the restatement's."""
    from multimodal_embeddings_amd._lib import lanczos_tables

    for in_size, out_size in ((case["w"], case["new_w"]), (case["h"], case["new_h"])):
        if in_size == out_size:
            continue
        b, k = lanczos_tables(in_size, out_size)
        rb, rk = ref.tables(in_size, out_size)
        assert k.shape == rk.shape == (out_size, ref.ksize_of(in_size, out_size))
        assert np.array_equal(b, rb) and np.array_equal(k, rk)
    img = ref.make_image(case["seed"], case["h"], case["w"], "noise")
    got = ref.resize_with_tables(img, case["new_h"], case["new_w"], tables_fn=lanczos_tables)
    assert _sha(got) == _sha(_pillow(img, case["new_h"], case["new_w"]))


# ---- (c) coefficient bounds ------------------------------------------------------------------------------------------------
# The kernels multiply a pixel byte by a coefficient with a signed 24-bit multiply and sum in signed 32 bits from 2^21, so
# they need |k| <= 2^23 - 1 and 255 * sum |k| + 2^21 <= 2^31 - 1 for EVERY row of every accepted (in, out).  With the real
# weights w_j = lanczos(t_j), t_j = (j + 0.5 - c) / fs over the taps 0 <= j < in, A = sum |w_j| and W = sum w_j, a row's
# coefficients are round(w_j / W * 2^22), so |k| <= A / W * 2^22 + 0.5 and sum |k| <= A / W * 2^22 + 0.5 * 97: both needs
# follow from A / W < RATIO_MAX = 1.99 (1.99 * 2^22 + 48.5 = 8 346 714 < (2^31 - 1 - 2^21) / 255 = 8 413 552 < 2^23).
#
# A row depends on (in, out, xx) only through fs = max(in / out, 1), the centre c = (xx + 0.5) * in / out and the clip of
# the window at 0 and `in`.  The accepted range (in <= 32768, out <= 8000, in / out <= 16) is covered by three parts:
#   1. in <= 98, down-scaling (in / 16 <= out < in): EVERY pair, every row, exactly, from the tables themselves.  A window
#      can be clipped on both sides only when in < 6 fs + 2 <= 98 (down) -- this part -- or in < 8 with fs = 1 (part 2).
#   2. up-scaling (fs = 1, c anywhere in (0, in)): in = 1..8 and the one-sided clip, a one-dimensional cover of c.
#   3. in >= 99, down-scaling: one clip at most; the right one mirrors the left (lanczos is even), so c in
#      [fs / 2, 3 fs + 1.5] with taps j >= 0 covers the clipped rows and every phase of the unclipped ones, for ALL real
#      fs in [1, 16], a superset of the ratios in / out.
# Parts 2 and 3 are covers of a continuous domain, not samples: a cell (fs +- dfs, c +- dc) is accepted when
# (A + e) / (W - e) < RATIO_MAX at its centre, where e bounds the change of A and of W inside the cell, and is split in four
# otherwise (a cell that small that it cannot be split any more fails the test).  e: inside the cell every tap moves by
# |dt| <= (dc + 3 dfs) / fs_lo (only taps with |t| < 3 in one of the two configurations count, lanczos(+-3) = 0); at most
# 2 (6 fs_hi + 1) taps count; lanczos = s(x) s(x / 3) with s(x) = sin(pi x) / (pi x), |s| <= 1, |s'| <= pi / 2, so
# |lanczos'| <= pi / 2 + pi / 6 < 2.1, and |lanczos| has the same Lipschitz constant.
RATIO_MAX = 1.99
LIP = 2.1


def _lanczos_np(t):
    t = np.asarray(t, dtype=np.float64)
    out = np.sinc(t) * np.sinc(t / 3.0)  # numpy's sinc is sin(pi x) / (pi x); its last-bit differences are far inside e
    return np.where((t >= -3.0) & (t < 3.0), out, 0.0)


def _row_sums(fs, c, in_size):
    """A = sum |w|, W = sum w over the taps 0 <= j < in_size (None: no right clip) for arrays of (fs, c)."""
    fs = np.asarray(fs, dtype=np.float64)[:, None]
    c = np.asarray(c, dtype=np.float64)[:, None]
    jmax = int(np.ceil((c + 3.0 * fs).max())) + 1
    if in_size is not None:
        jmax = min(jmax, in_size)
    j = np.arange(jmax, dtype=np.float64)[None, :]
    w = _lanczos_np((j + 0.5 - c) / fs)
    return np.abs(w).sum(axis=1), w.sum(axis=1)


def _cover(cells, in_size, max_depth=12):
    """cells: float array [n, 4] (fs_lo, fs_hi, c_lo, c_hi).  Accept or split until none is left; -> the largest
    (A + e) / (W - e) an accepted cell had."""
    worst = 0.0
    for depth in range(max_depth + 1):
        if len(cells) == 0:
            return worst
        bad = []
        for lo in range(0, len(cells), 20000):  # bounded memory
            part = cells[lo : lo + 20000]
            fs_lo, fs_hi, c_lo, c_hi = part.T
            fs, c = (fs_lo + fs_hi) / 2, (c_lo + c_hi) / 2
            A, W = _row_sums(fs, c, in_size)
            e = 2 * (6 * fs_hi + 1) * LIP * ((c_hi - c_lo) / 2 + 3 * (fs_hi - fs_lo) / 2) / fs_lo
            ok = (W - e > 0) & ((A + e) < RATIO_MAX * (W - e))
            if ok.any():
                worst = max(worst, float(((A + e) / (W - e))[ok].max()))
            bad.append(part[~ok])
        bad = np.concatenate(bad)
        if len(bad) == 0:
            return worst
        fs_lo, fs_hi, c_lo, c_hi = bad.T
        fm, cm = (fs_lo + fs_hi) / 2, (c_lo + c_hi) / 2
        if (fs_hi == fs_lo).all():  # one-dimensional cover: halves
            cells = np.concatenate([np.stack([fs_lo, fs_hi, c_lo, cm], 1), np.stack([fs_lo, fs_hi, cm, c_hi], 1)])
        else:
            cells = np.concatenate([np.stack([a, b, c0, c1], 1) for a, b in ((fs_lo, fm), (fm, fs_hi)) for c0, c1 in ((c_lo, cm), (cm, c_hi))])
    raise AssertionError(f"{len(cells)} cells could not be bounded below {RATIO_MAX}, e.g. (fs_lo, fs_hi, c_lo, c_hi) = {cells[0]}")


def test_coefficient_bounds_small_inputs_exactly(lib):
    """(c) part 1: every down-scaling pair with in <= 98, every row, from mme_lanczos_tables itself."""
    from multimodal_embeddings_amd._lib import lanczos_tables

    max_k = max_sum = 0
    for in_size in range(2, 99):
        for out_size in range((in_size + 15) // 16, in_size):
            _, k = lanczos_tables(in_size, out_size)
            max_k = max(max_k, int(np.abs(k).max()))
            max_sum = max(max_sum, int(np.abs(k).astype(np.int64).sum(axis=1).max()))
    print(f"in <= 98: max |k| = {max_k / 2**22:.4f} * 2^22, max sum |k| = {max_sum / 2**22:.4f} * 2^22")
    assert max_k <= 2**23 - 1
    assert 255 * max_sum + 2**21 <= 2**31 - 1


def test_coefficient_bounds_upscaling_cover():
    """(c) part 2: fs = 1, every centre c in (0, in) for in = 1..8, and the one-sided clip with every phase beyond."""
    worst = 0.0
    for in_size in list(range(1, 9)) + [None]:
        hi = 4.5 if in_size is None else float(in_size)
        edges = np.linspace(0.0, hi, int(hi * 64) + 1)
        cells = np.stack([np.ones(len(edges) - 1), np.ones(len(edges) - 1), edges[:-1], edges[1:]], 1)
        worst = max(worst, _cover(cells, in_size))
    print(f"up-scaling: (A + e) / (W - e) <= {worst:.4f}")
    assert worst < RATIO_MAX


def test_coefficient_bounds_downscaling_cover():
    """(c) part 3: every real fs in [1, 16] and every centre of a row with at most one clipped side."""
    fs_edges = np.exp(np.linspace(0.0, np.log(16.0), 257))
    cells = []
    for a, b in zip(fs_edges[:-1], fs_edges[1:]):
        # c from fs / 2 (the first row's centre) to 3 fs + 1.5 (no clip left, one whole period of the phase)
        c_edges = np.linspace(a / 2, 3 * b + 1.5, 129)
        cells.append(np.stack([np.full(128, a), np.full(128, b), c_edges[:-1], c_edges[1:]], 1))
    worst = _cover(np.concatenate(cells), None)
    print(f"down-scaling: (A + e) / (W - e) <= {worst:.4f}")
    assert worst < RATIO_MAX


def test_coefficient_bounds_of_the_recorded_cases(lib):
    """(c) the figures of the accepted extremes themselves: ratio 16 at the largest input, the cap at the largest side."""
    from multimodal_embeddings_amd._lib import lanczos_tables

    for in_size, out_size in ((32768, 2048), (32768, 8000), (8001, 8000), (16, 1), (1, 8000), (127999 // 16, 500)):
        _, k = lanczos_tables(in_size, out_size)
        assert int(np.abs(k).max()) <= 2**23 - 1
        assert 255 * int(np.abs(k).astype(np.int64).sum(axis=1).max()) + 2**21 <= 2**31 - 1


# ---- (d) the size rule ---------------------------------------------------------------------------------------------------
def test_size_rule():
    """int(size * (8000 / max(size))) in Python, as embedder.py:110-114 evaluates it: 7999 for some long sides, 0 for a
    one-pixel side; not "fixed"."""
    from multimodal_embeddings_amd.embedder import capped_size

    assert ref.capped_size(9000, 12000) == capped_size(9000, 12000) == (6000, 8000)
    assert capped_size(8311, 12) == (7999, 11)
    assert capped_size(1, 9000) == (0, 8000)  # Pillow refuses it: ValueError, a None hole in the embedder
    short = [s for s in range(8001, 40000) if int(s * (8000 / s)) == 7999]
    assert len(short) == 3755 and all(int(s * (8000 / s)) in (7999, 8000) for s in range(8001, 40000))
    for h, w in ((8311, 12), (12, 8311), (20000, 3), (8001, 8001)):
        from PIL import Image

        scale = 8000 / max(w, h)
        want = Image.new("RGB", (w, h)).resize((int(w * scale), int(h * scale)), Image.LANCZOS).size
        assert capped_size(h, w) == (want[1], want[0])


# ---- (e) refusals that need no device ----------------------------------------------------------------------------------------
def _err(lib):
    return lib.mme_last_error(None).decode()


def test_tables_refusals(lib):
    ks = C.c_int(-7)
    for args, words in (((0, 5), ("in_size = 0", "1..32768")), ((32769, 8000), ("in_size = 32769", "1..32768")),
                        ((100, 0), ("out_size = 0", "1..8000")), ((9000, 8001), ("out_size = 8001", "1..8000")),
                        ((1601, 100), ("in_size / out_size = 1601 / 100", "at most 16"))):
        assert lib.mme_lanczos_tables(*args, None, None, C.byref(ks)) == -1
        assert all(w in _err(lib) for w in words), _err(lib)
        assert ks.value == -7  # nothing is written
    assert lib.mme_lanczos_tables(100, 50, None, None, None) == -1 and "ksize is null" in _err(lib)
    b = np.full((50, 2), -1, dtype=np.int32)
    assert lib.mme_lanczos_tables(100, 50, b.ctypes.data, None, C.byref(ks)) == -1 and "both" in _err(lib)
    assert (b == -1).all()
    assert lib.mme_lanczos_tables(1600, 100, None, None, C.byref(ks)) == 0 and ks.value == 97
    assert lib.mme_lanczos_tables(9, 23, None, None, C.byref(ks)) == 0 and ks.value == 7


def test_workspace_refusals_and_size(lib):
    n = C.c_size_t(12345)
    for args, words in (((0, 5, 1, 5), ("h = 0", "1..32768")), ((5, 32769, 5, 8000), ("w = 32769", "1..32768")),
                        ((9000, 10, 8001, 8), ("new_h = 8001", "1..8000")), ((6, 9000, 5, 0), ("new_w = 0", "1..8000")),
                        ((17, 9, 1, 9), ("h / new_h = 17 / 1", "at most 16"))):
        assert lib.mme_lanczos_workspace(*args, C.byref(n)) == -1
        assert all(w in _err(lib) for w in words), _err(lib)
        assert n.value == 12345
    assert lib.mme_lanczos_workspace(6, 9000, 5, 8000, None) == -1 and "bytes is null" in _err(lib)
    assert lib.mme_lanczos_workspace(6, 9000, 5, 8000, C.byref(n)) == 0
    # the horizontal pass's image (16-byte-pitched rows) and both tables fit
    assert n.value >= 6 * 24000 + 8000 * (7 + 2) * 4 + 5 * (9 + 2) * 4


def test_python_checks_name_field_value_and_range():
    from multimodal_embeddings_amd._lib import MmeError, check_lanczos_geometry, lanczos_geometry_ok

    assert lanczos_geometry_ok(9000, 12000, 6000, 8000) and lanczos_geometry_ok(4, 32768, 1, 8000)
    assert not lanczos_geometry_ok(40000, 10, 8000, 2) and not lanczos_geometry_ok(17, 9, 1, 9)
    with pytest.raises(MmeError, match=r"h = 40000; supported 1\.\.32768"):
        check_lanczos_geometry(40000, 10, 8000, 2)
    with pytest.raises(MmeError, match=r"new_w = 8001; supported 1\.\.8000"):
        check_lanczos_geometry(10, 9000, 8, 8001)
    with pytest.raises(MmeError, match=r"h / new_h = 17 / 1; supported: a ratio of at most 16"):
        check_lanczos_geometry(17, 9, 1, 9)
