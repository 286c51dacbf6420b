"""Every pixel-normalisation form of the preprocessing kernels, bit for bit against the oracle.

`mme_set_normalisation` leads to four code paths: the host search of `set_lut` (capi.hip) for a per-channel pair (a, b) with
bf16(fma(u, a, b)) == bf16(table[u]) for all 256 u; the affine emitter of `resize_v_patchify<true>` when every channel has such
a pair; its table emitter when one has not; `resize_v_patchify<false>` (a batch of 224 x 224 crops only) and `resize_v_tiles`,
which always read the table.  The constant sets below reach each of them: sets whose pair is the starting pair, sets that
need a neighbour, sets with no pair at all.

Which emitter a set reaches is PREDICTED here by a restatement of the search that needs no device (`reference_search`: same
start values, same visiting order, same acceptance test, an fma made exact by rational arithmetic) and then read back from the
context (`Engine.normalisation_form`), so that no set can quietly take another form than the one it is listed for.  All of it
is exact arithmetic: there are no tolerances, every comparison is of bits.

The tests named `*_without_a_device` run on the CPU: they pin the reference (its table against the oracle's, its fma against a
case where rounding twice gives another answer), classify every set, and show that the oracle's patches of the test crops under
each set differ from what a kernel with the wrong constants would give -- the device tests cannot pass vacuously.
"""
import collections
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd.weights import f32_to_bf16_bits, round_to_bf16
from oracle import preprocess as opre

gpu = pytest.mark.gpu
F32 = np.float32


# ---- the constant sets --------------------------------------------------------------------------------------------------
# "draw k": the k-th draw (from 0) of rng = numpy.random.default_rng(0), each draw being
#     mean = round(rng.uniform(0, 1, 3), 4); std = round(rng.uniform(0.02, 1, 3), 4)
# (`test_the_seeded_sets_are_what_the_seed_gives_without_a_device` regenerates them).  The four `table_*` sets that are no
# draw are the candidates of a twice-rounded replay of the search; the exact reference confirms every one of them.
DRAWS = {
    "neighbour_a_down_b_up": 238, "neighbour_a_up_b_down": 1496, "neighbour_two_channels": 923, "table_ch2": 543,
}
SETS = {
    "clip": (opre.CLIP_MEAN, opre.CLIP_STD),
    "half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "identity": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "neighbour_a_down_b_up": ((0.9294, 0.3243, 0.32), (0.0491, 0.7069, 0.1258)),
    "neighbour_a_up_b_down": ((0.7451, 0.515, 0.1346), (0.2893, 0.6667, 0.6249)),
    "neighbour_two_channels": ((0.814, 0.2863, 0.3294), (0.7248, 0.7668, 0.201)),
    "table_ch0": ((0.6, 0.892, 0.7415), (0.1993, 0.0298, 0.0224)),
    "table_ch0_other": ((0.4, 0.5009, 0.8475), (0.3404, 0.5428, 0.3588)),
    "table_ch0_wide_std": ((0.6, 0.6098, 0.3081), (0.5918, 0.0807, 0.7326)),
    "table_ch1": ((0.5908, 0.5098, 0.7532), (0.2858, 0.101, 0.6727)),
    "table_ch2": ((0.8003, 0.658, 0.4902), (0.8925, 0.446, 0.2625)),
}
# What the search does per channel: (steps of a, steps of b) in f32 neighbours from the starting pair, signed; None = no pair
# among the 17 x 17 (the host stops at the first such channel: exact = 0, later channels are not searched).
EXPECTED_STEPS = {
    "clip": [(0, 0), (0, 0), (0, 0)],
    "half": [(0, 0), (0, 0), (0, 0)],
    "imagenet": [(0, 0), (0, 0), (0, 0)],
    "identity": [(0, 0), (0, 0), (0, 0)],
    "neighbour_a_down_b_up": [(-4, 3), (0, 0), (0, 0)],
    "neighbour_a_up_b_down": [(3, -2), (0, 0), (0, 0)],
    "neighbour_two_channels": [(0, 0), (0, 1), (0, 1)],
    "table_ch0": [None],
    "table_ch0_other": [None],
    "table_ch0_wide_std": [None],
    "table_ch1": [(0, 0), None],
    "table_ch2": [(0, 0), (0, 0), None],
}
NAMES = list(SETS)


def _f32x3(v):
    return np.array(v, dtype=F32)


# ---- the reference of the search: exact arithmetic on the rationals ------------------------------------------------------
def round_f32(q: Fraction) -> F32:
    """The f32 nearest to the rational q, ties to even (one rounding; gradual underflow; no overflow in this file's range)."""
    if q == 0:
        return F32(0.0)
    n, d = abs(q.numerator), q.denominator
    e = n.bit_length() - d.bit_length()  # 2^(e-1) < |q| < 2^(e+1)
    if Fraction(n, d) < Fraction(2) ** e:
        e -= 1  # now 2^e <= |q| < 2^(e+1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    m = round(Fraction(n, d) / ulp)  # Python rounds a Fraction half to even; m <= 2^24
    r = F32(float(m * ulp))  # m * ulp has at most 24 significant bits (2^24 * ulp is the next power of two): exact
    assert Fraction(float(r)) == m * ulp
    return -r if q < 0 else r


def fma_f32(u: int, a: F32, b: F32) -> F32:
    """f32(u * a + b) with ONE rounding: what std::fmaf on the host and v_fma_f32 in the emitter compute."""
    return round_f32(Fraction(int(u)) * Fraction(float(a)) + Fraction(float(b)))


def reference_lut(mean, std) -> np.ndarray:
    """set_lut's table f32[3, 256]: x = f32(f64(u) * (1 / 255)); f32(f32(x - mean) / std), each step rounded once."""
    m, s = _f32x3(mean), _f32x3(std)
    out = np.empty((3, 256), dtype=F32)
    for ch in range(3):
        for u in range(256):
            x = F32(float(u) * (1.0 / 255.0))  # the f64 product is Python's own, then one rounding to f32
            out[ch, u] = round_f32(Fraction(float(round_f32(Fraction(float(x)) - Fraction(float(m[ch]))))) / Fraction(float(s[ch])))
    return out


def _neighbour(x: F32, steps: int) -> F32:
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf if steps > 0 else -np.inf))
    return F32(x)


def _visiting_order():
    """0, -1, +1, -2, +2 ... -8, +8: `for d in 0..8: for sign in -1, +1` without the second zero."""
    return [sg * d for d in range(9) for sg in (-1, 1) if not (d == 0 and sg == 1)]


Search = collections.namedtuple("Search", "exact a b steps")


def _bf16_bits(x: F32) -> int:
    u = int(F32(x).view(np.uint32))
    return (u + 0x7FFF + ((u >> 16) & 1)) >> 16  # round to nearest even, as weights.f32_to_bf16_bits


def reference_search(mean, std) -> Search:
    """set_lut's search, restated: per channel from a0 = f32((1 / 255) / f64(std)), b0 = f32(-f64(mean) / f64(std)), the
    slope's neighbours in the outer loop and the offset's in the inner one, nearest first and downwards before upwards;
    the first pair with bf16(fma(u, a, b)) == bf16(table[u]) for all 256 u is taken.  A channel without one ends it."""
    m, s = _f32x3(mean), _f32x3(std)
    want = f32_to_bf16_bits(reference_lut(mean, std))
    a_out, b_out, steps = np.zeros(3, dtype=F32), np.zeros(3, dtype=F32), []
    for ch in range(3):
        a0 = F32((1.0 / 255.0) / float(s[ch]))  # f64 arithmetic, one rounding to f32
        b0 = F32(-float(m[ch]) / float(s[ch]))
        found = None
        for da in _visiting_order():
            a = _neighbour(a0, da)
            for db in _visiting_order():
                b = _neighbour(b0, db)
                if all(_bf16_bits(fma_f32(u, a, b)) == int(want[ch, u]) for u in range(256)):
                    found = (da, db)
                    a_out[ch], b_out[ch] = a, b
                    break
            if found:
                break
        steps.append(found)
        if found is None:
            return Search(False, a_out, b_out, steps)
    return Search(True, a_out, b_out, steps)


@functools.lru_cache(maxsize=None)
def reference(name) -> Search:
    return reference_search(*SETS[name])


# ---- the crops, and the oracle's answer for every set --------------------------------------------------------------------
# The smallest shapes (h, w) that reach each branch of the vertical kernel: the aligned copy; no pass / one pass with padding
# columns, padding rows and all-padding bands; a vertical pass only; a horizontal pass only; both passes up-scaling and
# down-scaling; a single pixel; a near-square crop.  The last crop is planted: its three channels are three different
# constants, so that constants of one channel applied to another change every value of it.
SHAPES = [(224, 224), (224, 100), (100, 224), (500, 224), (224, 500), (20, 63), (63, 20), (448, 448), (300, 170), (1, 1), (223, 225)]
PLANTED = (37, 141, 232)


@functools.lru_cache(maxsize=None)
def crops():
    rng = np.random.default_rng(20)
    out = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    planted = np.empty((90, 50, 3), dtype=np.uint8)
    planted[:] = PLANTED
    return out + [planted]


@functools.lru_cache(maxsize=None)
def square_crops():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(3)]


# (16, 30) is there for the unused slots: at tile 16 it fills two of the four, the other shapes fill all of them
TILE_SHAPES = [(300, 170), (17, 90), (224, 224), (40, 33), (16, 30)]
TILE_GEOMETRIES = [(224, 1), (16, 4)]


@functools.lru_cache(maxsize=None)
def tile_crops():
    rng = np.random.default_rng(22)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in TILE_SHAPES]


@functools.lru_cache(maxsize=None)
def oracle_patches(name, square=False):
    """bf16-rounded oracle patches [196, 768] of every test crop under set `name` (computed once, never modified)."""
    mean, std = SETS[name]
    out = [round_to_bf16(opre.preprocess_to_patches(a, mean, std)) for a in (square_crops() if square else crops())]
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def canvases():
    """(u8 canvas [224, 224, 3], new_h, new_w) of every test crop: the oracle's steps before its table lookup."""
    out = []
    for a in crops():
        nh, nw = opre.fit_to_canvas(*a.shape[:2])
        c = np.zeros((224, 224, 3), dtype=np.uint8)
        c[:nh, :nw] = opre.pil_bilinear_resize_u8(a, nh, nw)
        out.append((c, nh, nw))
    return out


def patches_of(canvas, lut, pad=None, nh=224, nw=224):
    """bf16-rounded patches of a canvas under a table; `pad` f32[3] overrides the value of the padding outside nh x nw."""
    pv = np.stack([lut[c][canvas[:, :, c]] for c in range(3)])
    if pad is not None:
        for c in range(3):
            pv[c, nh:, :] = pad[c]
            pv[c, :, nw:] = pad[c]
    return round_to_bf16(opre.patchify(pv))


def _distinct_channels(name):
    mean, std = SETS[name]
    return len({(F32(m), F32(s)) for m, s in zip(mean, std)}) == 3


def _pack(arrays, device="cuda:0"):
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(arrays), dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(device), offs, hw


# ---- without a device ----------------------------------------------------------------------------------------------------
def test_exact_fma_rounds_once_without_a_device():
    """205 * (10475530 * 2^-55) + 1 = 1 + 2^-24 + 2^-54: just above the midpoint of 1 and its f32 successor.  An f64
    multiply-add lands ON the midpoint (2^-54 is a quarter of its ulp) and the second rounding then goes to even, 1.0;
    one rounding gives 1 + 2^-23.  Plus the rounding helper on ties, subnormals and signs."""
    a = F32(10475530 * 2.0**-55)
    assert float(a) == 10475530 * 2.0**-55
    assert F32(205.0 * float(a) + 1.0) == F32(1.0)  # the twice-rounded answer
    assert fma_f32(205, a, F32(1.0)) == F32(1.0 + 2.0**-23)
    assert round_f32(Fraction(1) + Fraction(1, 2**24)) == F32(1.0)  # tie to even, downwards
    assert round_f32(Fraction(1) + Fraction(3, 2**24)) == F32(1.0 + 2.0**-22)  # tie to even, upwards
    assert round_f32(-Fraction(1) - Fraction(3, 2**24)) == F32(-1.0 - 2.0**-22)
    assert round_f32(Fraction(3, 2**150)) == F32(2.0**-148) and round_f32(Fraction(1, 2**150)) == F32(0.0)  # subnormal ties
    rng = np.random.default_rng(5)
    for x in rng.standard_normal(200) * 10.0 ** rng.uniform(-6, 6, 200):  # an f64 -> f32 conversion is one rounding too
        assert round_f32(Fraction(float(x))) == F32(x)
    for u in (0, 1, 255):  # an fma whose exact result is an f32 is that f32
        assert fma_f32(u, F32(0.25), F32(-3.0)) == F32(u * 0.25 - 3.0)


def test_the_seeded_sets_are_what_the_seed_gives_without_a_device():
    rng = np.random.default_rng(0)
    wanted = {k: n for n, k in DRAWS.items()}
    for k in range(max(wanted) + 1):
        mean, std = np.round(rng.uniform(0, 1, 3), 4), np.round(rng.uniform(0.02, 1, 3), 4)
        if k in wanted:
            assert (tuple(mean.tolist()), tuple(std.tolist())) == SETS[wanted[k]], (k, wanted[k])


@pytest.mark.parametrize("name", NAMES)
def test_reference_classifies_the_set_without_a_device(name):
    """The reference's table is the oracle's, bit for bit; the search ends where this file says it ends; an accepted pair
    is the stated number of f32 neighbours away from the starting pair and reproduces all 256 table entries of its channel."""
    mean, std = SETS[name]
    lut = reference_lut(mean, std)
    assert np.array_equal(lut.view(np.uint32), opre.normalise_lut(mean, std).view(np.uint32))
    r = reference(name)
    print(name, "exact" if r.exact else "table", r.steps)
    assert r.steps == EXPECTED_STEPS[name]
    assert r.exact == (None not in r.steps)
    m, s = _f32x3(mean), _f32x3(std)
    for ch, st in enumerate(r.steps):
        if st is None:
            continue
        assert r.a[ch] == _neighbour(F32((1.0 / 255.0) / float(s[ch])), st[0]) and r.b[ch] == _neighbour(F32(-float(m[ch]) / float(s[ch])), st[1])
        got = np.array([fma_f32(u, r.a[ch], r.b[ch]) for u in range(256)], dtype=F32)
        assert np.array_equal(f32_to_bf16_bits(got), f32_to_bf16_bits(lut[ch]))


def test_the_list_has_every_kind_of_set_without_a_device():
    kinds = {n: reference(n).steps for n in NAMES}
    start = [n for n, st in kinds.items() if st == [(0, 0)] * 3]
    neighbour = [n for n, st in kinds.items() if None not in st and st != [(0, 0)] * 3]
    no_pair_ch0 = [n for n, st in kinds.items() if st == [None]]
    no_pair_later = [n for n, st in kinds.items() if None in st and len(st) > 1]
    print("starting pair:", start, "| neighbour pair:", neighbour, "| no pair on channel 0:", no_pair_ch0, "| no pair on channel 1 or 2:", no_pair_later)
    assert {"clip", "half", "imagenet", "identity"} <= set(start)
    assert neighbour and no_pair_ch0 and no_pair_later
    # a neighbour of the slope in each direction, one of the offset alone, and two channels of one set off the start
    moved = [st for n in neighbour for st in kinds[n] if st != (0, 0)]
    assert any(da < 0 for da, _ in moved) and any(da > 0 for da, _ in moved) and any(da == 0 and db != 0 for da, db in moved)
    assert any(sum(st != (0, 0) for st in kinds[n]) >= 2 for n in neighbour)
    # the channel mix-ups below need sets whose three channels differ, in either form
    assert any(_distinct_channels(n) for n in neighbour) and any(_distinct_channels(n) for n in no_pair_ch0 + no_pair_later)
    # and the test shapes: crops with and without padding, tile cases with padding inside the canvas and with unused slots
    assert any(nh < 224 or nw < 224 for _, nh, nw in canvases()) and any(nh == 224 and nw == 224 for _, nh, nw in canvases())
    unused = padded = 0
    for tile, mt in TILE_GEOMETRIES:
        for a in tile_crops():
            _, _, nt, (th, tw) = opre.preprocess_tiles(a, tile, mt)
            nh, nw = opre.fit_to_canvas_general(*a.shape[:2], th * tile, tw * tile, tile)
            unused += nt < mt
            padded += nh < th * tile or nw < tw * tile
    assert unused and padded, (unused, padded)


@pytest.mark.parametrize("name", NAMES)
def test_wrong_constants_are_separated_without_a_device(name):
    """What the device tests compare with tells the set's constants from the ways a kernel could get them wrong: per crop
    and per channel plane of the patches, the oracle differs in at least one element from the CLIP constants (a setter that
    did nothing), from the constants of the next channel and from those of channel 0 (a mix-up of channels; sets whose
    channels differ), and from padding left at the CLIP value (crops with padding)."""
    mean, std = SETS[name]
    lut, clip = opre.normalise_lut(mean, std), opre.normalise_lut()
    want = oracle_patches(name)
    mutants = {}
    if name != "clip":
        mutants["clip"] = (clip, None)
        mutants["clip_padding"] = (lut, clip[:, 0])
    if _distinct_channels(name):
        mutants["next_channel"] = (lut[[1, 2, 0]], None)
        mutants["channel_0"] = (lut[[0, 0, 0]], None)
    for k, (canvas, nh, nw) in enumerate(canvases()):
        assert np.array_equal(patches_of(canvas, lut), want[k]), k  # this helper is the oracle's own computation
        for mname, (mlut, pad) in mutants.items():
            if pad is not None and nh == 224 and nw == 224:
                continue
            diff = (patches_of(canvas, mlut, pad, nh, nw) != want[k]).reshape(196, 3, 256)
            for ch in range(3):
                if mname == "channel_0" and ch == 0:
                    continue
                assert diff[:, ch].any(), (name, mname, k, ch)
    if name != "clip":  # the all-224 batch: the same for its three crops
        for a, w in zip(square_crops(), oracle_patches(name, square=True)):
            assert (patches_of(a, clip) != w).reshape(196, 3, 256).any(axis=(0, 2)).all()


# ---- on the device -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)  # no weights: preprocessing does not ask for them
    yield e
    e.close()


def _restore(engine):
    engine.set_normalisation(opre.CLIP_MEAN, opre.CLIP_STD)


def _device_patches(engine, arrays):
    pix, offs, hw = _pack(arrays)
    patches = engine.preprocess(pix, offs, hw)
    torch.cuda.synchronize()
    return patches.float().cpu().numpy().reshape(len(arrays), 196, 768)


def _assert_patches(got, want, what):
    for k, w in enumerate(want):
        bad = got[k].view(np.uint32) != w.view(np.uint32)
        assert not bad.any(), (what, k, int(bad.sum()), "first at (patch, column)", tuple(np.argwhere(bad)[0]))


def _assert_form(engine, name):
    exact, a, b = engine.normalisation_form()
    r = reference(name)
    assert exact == r.exact, (name, exact, r.steps)
    if exact:
        assert np.array_equal(a.view(np.uint32), r.a.view(np.uint32)) and np.array_equal(b.view(np.uint32), r.b.view(np.uint32)), (name, a, b, r.a, r.b)
    return exact, a, b


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_form_is_the_predicted_one(engine, name):
    """The context reports the form and the pair the reference predicts, and the pair it reports reproduces the oracle's
    table after the bf16 rounding in all 768 entries -- computed here, whatever the host's own verification said."""
    try:
        engine.set_normalisation(*SETS[name])
        exact, a, b = _assert_form(engine, name)
        if exact:
            lut = opre.normalise_lut(*SETS[name])
            for ch in range(3):
                got = np.array([fma_f32(u, a[ch], b[ch]) for u in range(256)], dtype=F32)
                assert np.array_equal(f32_to_bf16_bits(got), f32_to_bf16_bits(lut[ch])), (name, ch)
    finally:
        _restore(engine)
    assert engine.normalisation_form()[0] is True  # the CLIP constants are back, in their affine form


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_resizing_batch_matches_the_oracle(engine, name):
    """`resize_v_patchify<true>`: every branch of the vertical kernel in one batch, under the emitter the set reaches."""
    try:
        engine.set_normalisation(*SETS[name])
        _assert_form(engine, name)
        got = _device_patches(engine, crops())
    finally:
        _restore(engine)
    _assert_patches(got, oracle_patches(name), name)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_all_224_batch_matches_the_oracle(engine, name):
    """`resize_v_patchify<false>`: three 224 x 224 crops alone in a call, the default constants included."""
    try:
        engine.set_normalisation(*SETS[name])
        got = _device_patches(engine, square_crops())
    finally:
        _restore(engine)
    _assert_patches(got, oracle_patches(name, square=True), name)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_tiles_match_the_oracle(engine, name):
    """`resize_v_tiles`: f32 pixel values, aspect ids and tile counts equal the oracle's; padding inside a used canvas is
    (0 - mean) / std of its channel, an unused tile slot is all zero."""
    mean, std = SETS[name]
    pad = (F32(0.0) - _f32x3(mean)) / _f32x3(std)
    arrays = tile_crops()
    try:
        engine.set_normalisation(mean, std)
        pix, offs, hw = _pack(arrays)
        results = []
        for tile, mt in TILE_GEOMETRIES:
            pv, ids, mask, nt = engine.preprocess_tiles(pix, offs, hw, tile, mt)
            torch.cuda.synchronize()
            results.append((tile, mt, pv.cpu().numpy(), ids, nt))
    finally:
        _restore(engine)
    for tile, mt, host, ids, nt in results:
        for k, a in enumerate(arrays):
            want, aid, n_t, (th, tw) = opre.preprocess_tiles(a, tile, mt, mean, std)
            assert int(ids[k]) == aid and nt[k] == n_t == th * tw, (name, tile, mt, k)
            assert np.array_equal(host[k].view(np.uint32), want.view(np.uint32)), (name, tile, mt, k)
            assert not host[k, n_t:].view(np.uint32).any(), (name, tile, mt, k)  # +0.0 in every bit
            nh, nw = opre.fit_to_canvas_general(*a.shape[:2], th * tile, tw * tile, tile)
            full = host[k, :n_t].reshape(th, tw, 3, tile, tile).transpose(2, 0, 3, 1, 4).reshape(3, th * tile, tw * tile)
            for ch in range(3):
                assert (full[ch, nh:, :] == pad[ch]).all() and (full[ch, :, nw:] == pad[ch]).all(), (name, tile, mt, k, ch)


@gpu
def test_constants_follow_every_call_on_one_context(engine):
    """Affine, table, affine again, then the CLIP constants set explicitly: each call's form and patches are its own."""
    steps = ["neighbour_a_down_b_up", "table_ch1", "neighbour_a_down_b_up", "clip"]
    assert [reference(n).exact for n in steps] == [True, False, True, True]
    got = []
    try:
        for n in steps:
            engine.set_normalisation(*SETS[n])
            _assert_form(engine, n)
            got.append(_device_patches(engine, crops()))
    finally:
        _restore(engine)
    for n, g in zip(steps, got):
        _assert_patches(g, oracle_patches(n), n)
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))


@gpu
@pytest.mark.parametrize("name", ["neighbour_a_up_b_down", "table_ch2"])
def test_refused_constants_change_nothing(engine, name):
    """std with a zero, a negative value or a NaN is refused, and the constants in force before -- not the default ones,
    in either form -- stay in force: the same form, the same pair, patches equal to their oracle."""
    from multimodal_embeddings_amd._lib import MmeError

    try:
        engine.set_normalisation(*SETS[name])
        before = _assert_form(engine, name)
        for ch, bad in [(0, 0.0), (1, -0.25), (2, float("nan")), (0, float("nan"))]:
            std = [0.5, 0.5, 0.5]
            std[ch] = bad
            with pytest.raises(MmeError):
                engine.set_normalisation((0.5, 0.5, 0.5), std)
            after = _assert_form(engine, name)
            assert after[0] == before[0] and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32)) and np.array_equal(after[2].view(np.uint32), before[2].view(np.uint32))
        got = _device_patches(engine, crops())
        tiles = engine.preprocess_tiles(*_pack(tile_crops()[:1]), 16, 4)[0].cpu().numpy()
    finally:
        _restore(engine)
    _assert_patches(got, oracle_patches(name), name)
    assert np.array_equal(tiles[0].view(np.uint32), opre.preprocess_tiles(tile_crops()[0], 16, 4, *SETS[name])[0].view(np.uint32))
