"""The two attention kernels, one launch at a time (mme_attention_apply), against a float64 reference on planted Q/K/V.

Reference: written here from the definition, not from kernel code.  Per (image, head), in float64 on the device:
s = q . k (Q carries dh^-0.5 log2 e, so s is a base-2 logit), p = 2^(s - rowmax), out = sum p v / sum p; the tile-ViT
attention masks (padding query, padding key) pairs (oracle.mllama_vision.padding_flags).  Every input is a bf16 value,
so the reference sees exactly the bits the kernel sees, and every output element of every row is compared.

Tolerance: |got - ref| <= 2^-8 |ref| + 2^-8 A, A = sum p |v| / sum p from the same float64 pass.  The kernels round at
two points: each probability to bf16 (relative 2^-9: at most 2^-9 A in the numerator, at most 2^-9 |ref| through a
denominator formed from the same or from the unrounded probabilities) and the output to bf16 (2^-9 |out|).  The f32
accumulation over at most 6432 terms and the hardware exp2 (~2^-22 relative) are orders of magnitude below that, so
2^-9 (A + 2 |ref|) bounds an exact kernel's error and 2^-8 (|ref| + A) covers it with a little room -- while a wrong
probability, a wrong mask or a lost rescale moves an output by far more (checked: below).

Sharpness: every planted case names a mutant -- a plausible kernel bug written as a change of the reference's scores
(the spike key dropped, K5's clamped padding rows 197..199 counted as keys, "any padding" masked instead of "both
padding", the keys before a rescale left at the old scale) -- and asserts that the mutant's output differs from the true
reference by at least 4x the tolerance on every planted row: the case would catch that bug.

Modes (mme_set_attention_mode): 0 exact; 1 fast, re-run exactly when the launch's guard was raised; 2 re-run forced.
Every case runs in all three: outputs finite and within tolerance, mode 2 bit-identical to mode 0, and a launch that
reports `redone` bit-identical to mode 0 as well.  Each family keeps at least one launch with redone == 0 in mode 1,
so the fast form's own output is checked and not only the re-run's.
"""
import pytest
import torch

from oracle.mllama_vision import padding_flags

pytestmark = pytest.mark.gpu

GEOM = {0: (197, 12, 64), 1: (6432, 16, 80)}  # tokens, heads, head dim
TOKP, TOK = 1608, 1601  # tile-ViT: tokens per tile (padded), real tokens per tile
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.set_attention_mode(1)
    e.close()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, scale, g):
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _random_qkv(kind, n, seed, q_scale):
    """Q ~ N(0, q_scale), K, V ~ N(0, 1), bf16; scores have a standard deviation of ~1..2 log2 units."""
    T, H, dh = GEOM[kind]
    g = _gen(seed)
    x = torch.empty((n * T, 3, H * dh), dtype=torch.bfloat16, device="cuda")
    x[:, 0] = _randn((n * T, H * dh), q_scale, g)
    x[:, 1] = _randn((n * T, H * dh), 1.0, g)
    x[:, 2] = _randn((n * T, H * dh), 1.0, g)
    return x.view(n * T, 3 * H * dh)


def _view(qkv, kind):
    """[n, T, 3 (q k v), H, dh] view of the fused activation."""
    T, H, dh = GEOM[kind]
    return qkv.view(-1, T, 3, H, dh)


def _split3(x):
    """float64 values -> three bf16 parts whose sum is x exactly (a planted score with up to 24 significant bits)."""
    hi = x.to(torch.bfloat16)
    mid = (x - hi.double()).to(torch.bfloat16)
    lo = (x - hi.double() - mid.double()).to(torch.bfloat16)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x), "planted score not representable in three bf16 parts"
    return hi, mid, lo


def _pad(kind, ntiles, img):
    T = GEOM[kind][0]
    if kind == 0:
        return torch.zeros(T, dtype=torch.bool, device="cuda")
    return padding_flags(int(ntiles[img])).to("cuda")


def mask_both(s, pad):
    return s.masked_fill(pad[:, None] & pad[None, :], float("-inf"))


def reference(qkv, kind, ntiles=None, items=None, mutant=None):
    """float64 (out, A), each [n, T, H, dh] (NaN outside `items`, a list of (image, head); default all).
    mutant(img, head, s, pad) -> masked scores replaces the true masking (a named kernel bug)."""
    T, H, dh = GEOM[kind]
    x = _view(qkv, kind)
    n = x.shape[0]
    out = torch.full((n, T, H, dh), float("nan"), dtype=torch.float64, device="cuda")
    A = out.clone()
    items = items if items is not None else [(i, h) for i in range(n) for h in range(H)]
    chunk = 4 if kind == 1 else 1024
    for c0 in range(0, len(items), chunk):
        part = items[c0 : c0 + chunk]
        ii = torch.tensor([i for i, _ in part], device="cuda")
        hh = torch.tensor([h for _, h in part], device="cuda")
        q = x[ii, :, 0, hh].double()  # [c, T, dh]
        k = x[ii, :, 1, hh].double()
        v = x[ii, :, 2, hh].double()
        s = q @ k.transpose(1, 2)
        for j, (i, h) in enumerate(part):
            pad = _pad(kind, ntiles, i)
            s[j] = mutant(i, h, s[j], pad) if mutant else mask_both(s[j], pad)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        del s
        l = p.sum(-1, keepdim=True)
        out[ii, :, hh] = (p @ v) / l
        A[ii, :, hh] = (p @ v.abs()) / l
        del p
    return out, A


def _tol(ref, A):
    return 2.0**-8 * (ref.abs() + A)


def check_close(got, ref, A, kind, what):
    T, H, dh = GEOM[kind]
    g = got.view(-1, T, H, dh).double()
    finite = torch.isfinite(g)
    if not finite.all():
        first = (~finite).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~finite).sum())} non-finite outputs, first at (img, token, head, dim) {first}")
    err = (g - ref).abs()
    tol = _tol(ref, A)
    bad = err > tol
    if bad.any():
        first = bad.nonzero()[0].tolist()
        i, t, h, d = first
        raise AssertionError(f"{what}: {int(bad.sum())} outputs out of tolerance (worst err/tol {float((err / tol).nan_to_num(posinf=1e30).max()):.3g}); "
                             f"first at (img, token, head, dim) {first}: got {float(g[i, t, h, d])!r} ref {float(ref[i, t, h, d])!r} tol {float(tol[i, t, h, d])!r}")


def check_sharp(qkv, kind, ntiles, ref, A, planted, mutant, name):
    """planted: list of (img, head, rows): the mutant leaves the tolerance by 4x on every one of those rows."""
    items = sorted({(i, h) for i, h, _ in planted})
    mref, _ = reference(qkv, kind, ntiles, items=items, mutant=mutant)
    tol = _tol(ref, A)
    for i, h, rows in planted:
        r = torch.as_tensor(rows, device="cuda")
        ratio = ((mref[i, r, h] - ref[i, r, h]).abs() / tol[i, r, h]).nan_to_num(nan=float("inf")).amax(-1)
        assert bool((ratio >= 4).all()), f"mutant '{name}' is not separated on (img {i}, head {h}): rows {rows} ratio {ratio.tolist()}"


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def run_modes(eng, qkv, kind, ntiles=None, **kw):
    """{mode: (out, redone)} with the mode-independent contract checked: mode 0 never redone, mode 2 always and
    bit-identical to mode 0, mode 1 bit-identical to mode 0 whenever it reports a re-run."""
    res = {}
    try:
        for mode in MODES:
            eng.set_attention_mode(mode)
            res[mode] = eng.attention(qkv, kind, ntiles, **kw)
    finally:
        eng.set_attention_mode(1)
    assert not res[0][1], "mode 0 reported a re-run"
    assert res[2][1], "mode 2 did not re-run"
    assert _same(res[2][0], res[0][0]), "mode 2 (forced re-run) differs from mode 0"
    if res[1][1]:
        assert _same(res[1][0], res[0][0]), "mode 1 reported a re-run but its output is not the exact kernel's"
    return res


def check_all(res, ref, A, kind, what):
    for mode, (out, redone) in res.items():
        check_close(out, ref, A, kind, f"{what}, mode {mode} (redone {int(redone)})")


# ---------------------------------------------------------------------------------------------------------------------
# K5: ViT-B/16, 197 tokens, 12 heads of 64


@pytest.mark.parametrize("n", [1, 3, 85, 86, 127, 128, 170, 171, 255, 256, 511, 512, 777])
def test_k5_random_every_hsplit_and_persistent_walk(eng, n):
    """Ordinary scores, distinct data for every (crop, head).  n covers every hsplit (12, 6, 4, 3, 2, 1: launch_attention
    picks the smallest with n * hsplit >= 512) and grids whose persistent walk crosses crops unevenly."""
    qkv = _random_qkv(0, n, 1000 + n, 0.25)
    res = run_modes(eng, qkv, 0)
    assert not res[1][1], "ordinary scores raised the fast form's guard"
    ref, A = reference(qkv, 0)
    check_all(res, ref, A, 0, f"K5 random n={n}")


K5_SPIKE_KEYS = (0, 31, 32, 191, 192, 196)
K5_SPIKE_ROWS = [0, 31, 32, 195, 196]


def test_k5_spikes_at_tile_and_padding_borders(eng):
    """Spike keys at the borders of the 32-key tiles (0 = the fast form's reference tile, 191 / 192, 196 = the last real
    key, whose clamped copies fill LDS rows 197..199) for queries at the borders of the query blocks; spike ~2/3 of the
    row's mass, so both dropping it and counting it 4x move the output."""
    n = 3
    qkv = _random_qkv(0, n, 7, 0.25)
    x = _view(qkv, 0)
    x[:, :, 1, :, 0] = 0.0  # dim 0 of K: zero except at the spike key
    planted, spike_of = [], {}
    for i in range(n):
        for h in range(12):
            key = K5_SPIKE_KEYS[(i * 12 + h) % len(K5_SPIKE_KEYS)]
            x[i, key, 1, h, 0] = 10.0
            x[i, K5_SPIKE_ROWS, 0, h, 0] = 1.0
            spike_of[(i, h)] = key
            planted.append((i, h, K5_SPIKE_ROWS))
    res = run_modes(eng, qkv, 0)
    assert not res[1][1]
    ref, A = reference(qkv, 0)
    check_all(res, ref, A, 0, "K5 spikes")

    def dropped(i, h, s, pad):
        s = s.clone()
        s[:, spike_of[(i, h)]] = float("-inf")
        return s

    def pad_rows_counted(i, h, s, pad):  # rows 197..199 hold copies of key 196: counted, key 196 weighs 4x
        s = s.clone()
        s[:, 196] += 2.0
        return s

    check_sharp(qkv, 0, None, ref, A, planted, dropped, "spike key dropped")
    check_sharp(qkv, 0, None, ref, A, [p for p in planted if spike_of[p[:2]] == 196], pad_rows_counted, "padding rows 197..199 counted")


K5_RANGE_ROWS = [40, 100, 196]


def _k5_range_case(jump, v_abs, seed):
    """One crop; head 3, rows 40 / 100 / 196: scores = dim 0 of K exactly (Q = e0), -|N(0,1)| everywhere, 0 at key 5
    (the tile-0 maximum), `jump` at key 150; V of key 150 = +-v_abs (else ordinary)."""
    qkv = _random_qkv(0, 1, seed, 0.25)
    x = _view(qkv, 0)
    g = _gen(seed + 1)
    h = 3
    x[0, :, 0, h, 0] = 0.0
    x[0, K5_RANGE_ROWS, 0, h, :] = 0.0
    x[0, K5_RANGE_ROWS, 0, h, 0] = 1.0
    x[0, :, 1, h, 0] = -_randn((197,), 1.0, g).abs()
    x[0, 5, 1, h, 0] = 0.0
    x[0, 150, 1, h, 0] = jump
    if v_abs is not None:
        sign = torch.randint(0, 2, (64,), generator=g, device="cuda") * 2 - 1
        x[0, 150, 2, h, :] = (sign * v_abs).to(torch.bfloat16)
    return qkv, [(0, h, K5_RANGE_ROWS)]


@pytest.mark.parametrize("jump,v_abs,expect_redone", [(99.5, None, False), (100.5, None, True), (99.0, 2.0**29, None)],
                         ids=["jump99.5_no_redo", "jump100.5_redo", "jump99_v2^29_overflow"])
def test_k5_fast_form_range(eng, jump, v_abs, expect_redone):
    """The fast form's reference point is the maximum over key tile 0; its guard is per launch (one launch per case).
    99.5 above it: the sum stays below 2^100, the fast output stands and is checked.  100.5: the guard fires.  99 with
    |v| = 2^29 at the spike: P v passes f32's range while the sum does not -- O must not leave the kernel inf / NaN."""
    qkv, planted = _k5_range_case(jump, v_abs, 31)
    res = run_modes(eng, qkv, 0)
    ref, A = reference(qkv, 0)
    check_all(res, ref, A, 0, f"K5 jump {jump} |v| {v_abs}")
    if expect_redone is not None:
        assert res[1][1] == expect_redone, res[1][1]

    def dropped(i, hd, s, pad):
        s = s.clone()
        s[:, 150] = float("-inf")
        return s

    check_sharp(qkv, 0, None, ref, A, planted, dropped, "spike key dropped")


def test_k5_only_block_and_reverse_walk(eng):
    """only_block b: rows 32b..32b+31 of every crop are bit-identical to the full launch, every other row of a
    sentinel-filled `out` is untouched; reverse = 1 (the blocks walked from the last crop down) is bit-identical."""
    from multimodal_embeddings_amd._lib import MmeError

    for n in (3, 300):  # hsplit 12 / 2 (300 crops: an uneven persistent walk)
        qkv = _random_qkv(0, n, 50 + n, 0.25)
        try:
            for mode in MODES:
                eng.set_attention_mode(mode)
                full, _ = eng.attention(qkv, 0)
                rev, _ = eng.attention(qkv, 0, reverse=True)
                assert _same(rev, full), (n, mode)
                for b in range(7) if n == 3 else (0, 6):
                    out = torch.full_like(full, -12345.0)
                    sentinel = out.clone()
                    eng.attention(qkv, 0, only_block=b, out=out)
                    rows = torch.zeros(197, dtype=torch.bool, device="cuda")
                    rows[32 * b : 32 * b + 32] = True
                    rows = rows.repeat(n)
                    assert _same(out[rows], full[rows]), (n, mode, b)
                    assert _same(out[~rows], sentinel[~rows]), (n, mode, b)
        finally:
            eng.set_attention_mode(1)
    with pytest.raises(MmeError):
        eng.attention(qkv, 0, only_block=7)
    with pytest.raises(MmeError):
        eng.attention(_random_qkv(1, 1, 1, 0.1), 1, [4], only_block=0)
    with pytest.raises(MmeError):
        eng.attention(_random_qkv(1, 1, 1, 0.1), 1, [5])
    with pytest.raises(MmeError):
        eng.attention(_random_qkv(1, 1, 1, 0.1), 1, None)


# ---------------------------------------------------------------------------------------------------------------------
# tile-ViT: 6432 tokens (4 tiles x 1608, 1601 real), 16 heads of 80


def _is_pad(tok, nt):
    return tok % TOKP >= TOK or tok // TOKP >= nt


TV_PAD_ROWS = [0, 1599, 1600, 1601, 1607, 1608, 3215, 3216, 4000, 6431]


def test_tile_padding_borders(eng):
    """Four images using 3, 1, 4 and 2 tiles in one launch.  Spike keys at the tile borders {1599, 1600 (last real),
    1601, 1607 (padding), 1608, 3215, 3216, 6431 (the last key, alone in the 32-key last tile)} and at the first key of a
    padding tile, for real and padding queries: a padding key counts for a real query, not for a padding query."""
    ntiles = [3, 1, 4, 2]
    n = len(ntiles)
    qkv = _random_qkv(1, n, 11, 0.125)
    x = _view(qkv, 1)
    x[:, :, 1, :, 0] = 0.0
    spike_of, by_mutant = {}, {"drop": [], "any": [], "none": []}
    for i, nt in enumerate(ntiles):
        keys = [1599, 1600, 1601, 1607, 1608, 3215, 3216, 6431, nt * TOKP if nt < 4 else 4823]
        for h in range(16):
            key = keys[(h + i) % len(keys)]
            spike_of[(i, h)] = key
            x[i, key, 1, h, 0] = 13.0
            x[i, TV_PAD_ROWS, 0, h, 0] = 1.0
            kp = _is_pad(key, nt)
            for q in TV_PAD_ROWS:
                qp = _is_pad(q, nt)
                by_mutant["drop" if not kp else ("none" if qp else "any")].append((i, h, [q]))
    res = run_modes(eng, qkv, 1, ntiles)
    assert not res[1][1], "ordinary scores raised the fast form's guard"
    ref, A = reference(qkv, 1, ntiles)
    check_all(res, ref, A, 1, "tile padding borders")

    def dropped(i, h, s, pad):
        s = mask_both(s, pad)
        s[:, spike_of[(i, h)]] = float("-inf")
        return s

    def any_padding(i, h, s, pad):
        return s.masked_fill(pad[:, None] | pad[None, :], float("-inf"))

    def no_mask(i, h, s, pad):
        return s

    for name, fn in (("drop", dropped), ("any", any_padding), ("none", no_mask)):
        assert by_mutant[name], name
        check_sharp(qkv, 1, ntiles, ref, A, by_mutant[name], fn, {"drop": "spike key dropped", "any": "any padding masked",
                                                                   "none": "padding pair counted"}[name])


# queries of waves 0..3 (q mod 256 < 128) and of waves 4..7 (>= 128: they carry P across the barrier), all real tokens
TV_RESCALE_ROWS = [3, 77, 130, 250, 1000, 1200, 3300, 3350, 6000, 6100]


def test_tile_exact_rescale_positions(eng):
    """The exact kernel moves its running maximum (rescaling O and the sum) only when a granule's maximum rises more
    than DEFER = 8 above it.  Jumps of 7.875, 8.125 and 30 in granule 0 or 1 of key tiles 0, 1, 25 and 50 (the last,
    32 keys), for queries of both wave groups; rows see scores = dim 0 of K exactly (Q = e0): -|N(0,1)| with 0 at key 0."""
    ntiles = [4, 4, 4, 3]
    n = len(ntiles)
    qkv = _random_qkv(1, n, 21, 0.125)
    x = _view(qkv, 1)
    g = _gen(22)
    cases = [(j, t, gr) for j in (7.875, 8.125, 30.0) for t, gr in ((0, 0), (0, 1), (1, 0), (1, 1), (25, 0), (25, 1), (50, 0))]
    spike_of, stale, dropped_rows = {}, [], []
    for c, (jump, tile, gran) in enumerate(cases):
        i, h = divmod(c, 16)
        k0 = tile * 128 + gran * 64
        key = k0 + 17
        x[i, :, 0, h, 0] = 0.0
        x[i, TV_RESCALE_ROWS, 0, h, :] = 0.0
        x[i, TV_RESCALE_ROWS, 0, h, 0] = 1.0
        x[i, :, 1, h, 0] = -_randn((6432,), 1.0, g).abs()
        x[i, 0, 1, h, 0] = 0.0
        x[i, key, 1, h, 0] = jump
        spike_of[(i, h)] = (key, k0, jump)
        (stale if k0 > 0 else dropped_rows).append((i, h, TV_RESCALE_ROWS))
    res = run_modes(eng, qkv, 1, ntiles)
    assert not res[1][1], "ordinary scores raised the fast form's guard"
    ref, A = reference(qkv, 1, ntiles)
    check_all(res, ref, A, 1, "tile rescale positions")

    def stale_scale(i, h, s, pad):  # the keys before the jump's granule not rescaled: too heavy by 2^jump
        key, k0, jump = spike_of[(i, h)]
        s = mask_both(s, pad)
        s[TV_RESCALE_ROWS, :k0] += jump
        return s

    def dropped(i, h, s, pad):
        s = mask_both(s, pad)
        s[:, spike_of[(i, h)][0]] = float("-inf")
        return s

    check_sharp(qkv, 1, ntiles, ref, A, stale, stale_scale, "spike's P left at the old scale")
    check_sharp(qkv, 1, ntiles, ref, A, dropped_rows, dropped, "spike key dropped")


# queries of both wave groups, real tokens of a 4-tile image
TV_RANGE_ROWS = [0, 200, 3000, 5000, 6000]
_TV_RANGE_BASE = {}


def _tv_range_case(scores, spike_key, v_abs, seed):
    """One 4-tile image; head 0, rows TV_RANGE_ROWS: Q = e0 + e1 + e2, so a row's scores are the planted float64 values
    (three bf16 parts in K dims 0..2); the other heads are the same random data in every case (their reference is
    computed once).  V of the spike key = +-v_abs."""
    if "qkv" not in _TV_RANGE_BASE:
        qkv = _random_qkv(1, 1, 41, 0.125)
        ref, A = reference(qkv, 1, [4], items=[(0, h) for h in range(1, 16)])
        _TV_RANGE_BASE.update(qkv=qkv, ref=ref, A=A)
    qkv = _TV_RANGE_BASE["qkv"].clone()
    x = _view(qkv, 1)
    x[0, :, 0, 0, 0:3] = 0.0
    x[0, TV_RANGE_ROWS, 0, 0, :] = 0.0
    x[0, TV_RANGE_ROWS, 0, 0, 0:3] = 1.0
    hi, mid, lo = _split3(scores)
    x[0, :, 1, 0, 0], x[0, :, 1, 0, 1], x[0, :, 1, 0, 2] = hi, mid, lo
    if spike_key is not None:
        g = _gen(seed)
        sign = torch.randint(0, 2, (80,), generator=g, device="cuda") * 2 - 1
        x[0, spike_key, 2, 0, :] = (sign * v_abs).to(torch.bfloat16)
    ref, A = reference(qkv, 1, [4], items=[(0, 0)])
    ref[0, :, 1:], A[0, :, 1:] = _TV_RANGE_BASE["ref"][0, :, 1:], _TV_RANGE_BASE["A"][0, :, 1:]
    return qkv, ref, A


def _background(seed):
    """-|N(0,1)| per key, quantised to 1/256 (so that a planted score plus it stays exact in three bf16 parts), 0 at key 0."""
    g = _gen(seed)
    b = -(torch.randn(6432, generator=g, device="cuda", dtype=torch.float64).abs() * 256).round() / 256
    b[0] = 0.0
    return b


def test_tile_fast_form_staircase_recentres_every_tile(eng):
    """Scores rise by 50 per 128-key tile: the fast form's row sum passes 2^60 after every tile and the reference is
    re-centred 50 times; no re-run, the fast output is checked."""
    scores = _background(60) + 50.0 * (torch.arange(6432, device="cuda", dtype=torch.float64) // 128)
    qkv, ref, A = _tv_range_case(scores, None, None, 61)
    res = run_modes(eng, qkv, 1, [4])
    check_all(res, ref, A, 1, "tile staircase")
    assert not res[1][1], "a +50 staircase re-centres; it must not need the exact re-run"

    def stale_scale(i, h, s, pad):  # the last re-centring lost: every key before the last tile 2^50 too heavy
        s = s.clone()
        s[TV_RANGE_ROWS, :6400] += 50.0
        return s

    check_sharp(qkv, 1, [4], ref, A, [(0, 0, TV_RANGE_ROWS)], stale_scale, "spike's P left at the old scale")


FILLER = 59.75  # one key of tile 1: the row sum ends tile 1 just under 2^60, so the reference is not re-centred


@pytest.mark.parametrize("start", ["deep", "fresh"])
def test_tile_fast_form_one_tile_jump(eng, start):
    """A single score J above the running maximum, J in {60, 64, 66, 67, 68, 70, 127, 129}, V of that key +-|v| with
    |v| in {1, 4, 64}; one launch each (the guard is per launch).
      deep:  tile 1 holds one key at 59.75 above the first 32 keys' maximum (the row sum ends tile 1 just under 2^60: no
             re-centring), the jump comes in tile 2 -- the reference point sits as far below the running maximum as
             re-centring allows, so P = 2^(59.75 + J): the row sum overflows only for J > 68, but P |v| from J ~ 66.
      fresh: the jump comes in tile 1, the reference point is the maximum of the first 32 keys.
    Outputs finite and within tolerance in every mode; where the guard did not fire, the fast output itself is checked."""
    failures, kept = [], 0
    for J in (60.0, 64.0, 66.0, 67.0, 68.0, 70.0, 127.0, 129.0):
        for v_abs in (1.0, 4.0, 64.0):
            scores = _background(70)
            if start == "deep":
                scores[150] = FILLER
                key, top = 300, FILLER + J
            else:
                key, top = 200, J
            scores[key] = top
            qkv, ref, A = _tv_range_case(scores, key, v_abs, int(J) * 10 + int(v_abs))
            res = run_modes(eng, qkv, 1, [4])
            for mode, (out, redone) in res.items():
                try:
                    check_close(out, ref, A, 1, f"{start} J={J:g} |v|={v_abs:g} mode {mode} (redone {int(redone)})")
                except AssertionError as e:
                    failures.append(str(e))
            kept += not res[1][1]

            def dropped(i, h, s, pad, key=key):
                s = s.clone()
                s[:, key] = float("-inf")
                return s

            check_sharp(qkv, 1, [4], ref, A, [(0, 0, TV_RANGE_ROWS)], dropped, "spike key dropped")
    assert not failures, "\n".join(failures)
    assert kept > 0, "every case re-ran: the fast form's own output was never checked"


# ---- the stamped build (mme_attention_stamps): the only instantiations of K5 no other test launches --------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_k5_stamped_build_runs_and_fills_its_slots(eng, mode):
    """Engine.attention_stamps times the product kernel and runs the stamped build of the same form once (mode 0: the exact
    kernel, mode 1: the fast one).  Layout (mme.h): [workgroup = crop][wave][slot]; slot 7 = heads processed; waves 0..6
    compute (slot 3 = S^T, slot 5 = P.V); wave 7 only stages: no S^T, and its slots 5 / 6 carry the workgroup's clock pair."""
    heads = GEOM[0][1]
    try:
        eng.set_attention_mode(mode)
        _, st = eng.attention_stamps(B=2, iters=1)
    finally:
        eng.set_attention_mode(1)
    assert st.shape == (2, 8, 8)
    assert (st[:, :, 7] == heads).all(), st[:, :, 7]
    assert (st[:, :7, 3] > 0).all() and (st[:, :7, 5] > 0).all(), st[:, :7, (3, 5)]
    assert (st[:, 7, 5] > 0).all() and (st[:, 7, 6] > 0).all() and (st[:, 7, 3] == 0).all(), st[:, 7]
