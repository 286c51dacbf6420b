"""K1 on the device at the shapes the host plan's sweep shows to be extreme (tests/golden/k1_extreme_shapes.json, derived and
held current by tests/test_k1_plan_cpu.py), not at shapes someone guessed: per rule the largest tap capacities, LDS request and
scratch image, both neighbours of each class boundary of the horizontal pass (8 / 7 and 4 / 3 rows beside the table), the
smallest and largest resized sizes, every (kept / enlarged / reduced) combination of the two axes that occurs -- among them form
(c) of resize_v_patchify with a vertical pass (width kept, height filtered) -- the CLIP rule's largest source-row window and its
one-row window, and the corners of the domain.

Per rule and pattern (seeded noise; 0 / 255 columns, where a dropped or doubled tap moves a value by far more than one code) one
batch holds the rule's shapes of at most 4 M pixels and another the few whose extreme no smaller shape attains (the JSON marks
them; the Python reference of a 64 M pixel crop takes seconds, which is why they stand apart).  Every batch
  * is compared bit for bit with the oracle of its rule: oracle.preprocess.preprocess_to_patches (fit-and-pad),
    clip_preprocess_reference / resize_spec_reference (CLIP's rule and two specs), oracle.preprocess.preprocess_tiles (560, 4);
  * writes between sentinel rows that must be unchanged afterwards;
  * runs twice: packed at 16-byte aligned offsets, and packed tightly with consecutive crops starting at byte offsets congruent
    to 1, 2, 3, 5, 7, 9, 11, 13, 15 mod 16 in a buffer with 16 bytes of slack -- include/mme.h admits any byte offset, and the two
    outputs must be equal in bits;
  * agrees with Engine.k1_plan where the run shows it: no crop of these batches is flagged, the tile grids are the plan's, and a
    refused batch names the crop the plan flags.
The coefficient stride of the vertical pass is the batch's largest kv: a batch whose only large-kv crop stands last and one where
it stands first must give the other crops the same bits.

Measured on the MI355X: the module 17 s; a batch of up to 4 M pixel shapes at most 0.7 s (tiles), a batch of the 64 M pixel
shapes 0.6 s (fit-and-pad, one crop) to 2.1 s (CLIP's rule and the tiles, three crops each), most of it the Python reference.
Nothing differed: every rule is bit-exact at its extremes, and the tight packing gives the aligned packing's bits.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import clip_preprocess_reference as cpr  # noqa: E402
import k1_plan_reference as kref  # noqa: E402
import resize_spec_reference as rsr  # noqa: E402
from test_gpu_clip_preprocess import bf16_bits  # noqa: E402

from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from oracle import preprocess as opre  # noqa: E402

pytestmark = pytest.mark.gpu

RULES = ("fit_pad", "clip", "edge256_bicubic", "exact224_bilinear", "tiles560")
EXTREMES = json.load(open(os.path.join(HERE, "golden", "k1_extreme_shapes.json")))["rules"]
PIXEL_CAP = 4_000_000
TIGHT = (1, 2, 3, 5, 7, 9, 11, 13, 15)  # byte offsets mod 16 of consecutive crops in the tight packing
SENT16 = 0x7FB7  # a bf16 NaN no normalised pixel is
NAN_BITS = 0x7FC0BEEF
GUARD_ROWS = 8  # sentinel patch rows (768 bf16) before and behind the patch matrix
GUARD = 4096  # sentinel words before and behind the tile output


def shapes_of(rule, big):
    """the rule's distinct shapes in the JSON's order, of at most 4 M pixels or above"""
    out = []
    for row in EXTREMES[rule]:
        s = (row["h"], row["w"])
        assert (s[0] * s[1] > PIXEL_CAP) == bool(row.get("over_4M")), row
        if (s[0] * s[1] > PIXEL_CAP) == big and s not in out:
            out.append(s)
    return out


def image(pattern, h, w):
    rng = np.random.default_rng(h * 8191 + w)
    if pattern == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    cols = (rng.integers(0, 2, w) * 255).astype(np.uint8)  # 0 / 255 columns
    return np.ascontiguousarray(np.broadcast_to(cols[None, :, None], (h, w, 3)))


def pack(arrays, tight):
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(arrays), dtype=np.int64)
    end = 0
    for i, s in enumerate(sizes):
        want = TIGHT[i % len(TIGHT)] if tight else 0
        offs[i] = end + (want - end) % 16  # the first offset at or behind the previous crop's end with that residue
        end = offs[i] + s
    buf = np.zeros(int(end) + 16, dtype=np.uint8)  # 16 bytes of slack behind the last pixel
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    if tight:
        assert [int(o % 16) for o in offs] == [TIGHT[i % len(TIGHT)] for i in range(len(offs))] and (np.diff(offs) - sizes[:-1] < 16).all()
    return torch.from_numpy(buf).cuda(), offs, hw


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def set_rule(eng, rule):
    if rule in ("fit_pad", "clip"):
        eng.set_resize_rule(rule)
    else:
        eng.set_resize_spec(kref.RULES[rule][1])


def run_patches(eng, pix, offs, hw):
    """mme_preprocess into a patch matrix between sentinel rows -> uint16 [n, 196, 768]"""
    n = len(offs)
    rows = n * 196
    raw = torch.full(((rows + 2 * GUARD_ROWS) * 768,), SENT16, dtype=torch.int16, device="cuda")
    out = raw.view(rows + 2 * GUARD_ROWS, 768)[GUARD_ROWS : GUARD_ROWS + rows]
    offs, hw = eng._crop_tables(offs, hw)
    eng._check(eng.lib.mme_preprocess(eng.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, out.data_ptr(), eng._stream()), "mme_preprocess")
    torch.cuda.synchronize()
    host = raw.cpu().numpy().view(np.uint16).reshape(rows + 2 * GUARD_ROWS, 768)
    sent = np.uint16(SENT16 & 0xFFFF)
    assert (host[:GUARD_ROWS] == sent).all() and (host[-GUARD_ROWS:] == sent).all(), "written outside the patch matrix"
    return host[GUARD_ROWS:-GUARD_ROWS].reshape(n, 196, 768)


def run_tiles(eng, pix, offs, hw, tile=560, max_tiles=4):
    n = len(offs)
    words = n * max_tiles * 3 * tile * tile
    flat = torch.full((words + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    out = flat[GUARD : GUARD + words].view(n, max_tiles, 3, tile, tile)
    _, ids, _, nt = eng.preprocess_tiles(pix, offs, hw, tile, max_tiles, out=out)
    torch.cuda.synchronize()
    bits = flat.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (bits[:GUARD] == NAN_BITS).all() and (bits[-GUARD:] == NAN_BITS).all(), "written outside [n, max_tiles, 3, T, T]"
    return bits[GUARD:-GUARD].reshape(n, max_tiles, 3, tile, tile), ids, nt


def expected_patches(rule, img, lut):
    if rule == "fit_pad":
        return bf16_bits(opre.preprocess_to_patches(img))
    win = cpr.clip_window_u8(img) if rule == "clip" else rsr.spec_window_u8(kref.RULES[rule][1], img)
    return bf16_bits(opre.patchify(np.stack([lut[c][win[:, :, c]] for c in range(3)])))


def check_against_the_plan(rule, shapes):
    rec, _ = Engine.k1_plan(*_plan_args(rule), np.array(shapes, dtype=np.int32))
    assert not rec["refused"].any(), (rule, [s for s, r in zip(shapes, rec["refused"]) if r])
    return rec


def _plan_args(rule):
    arg, kw = kref.engine_rule(kref.RULES[rule])
    assert not kw or kw == {"tile": 560, "max_tiles": 4}
    return (arg,)


# (the exact 224 x 224 target attains every extreme below 4 M pixels: it has no second batch)
BATCHES = [(rule, pattern, big) for rule in RULES for pattern in ("noise", "binary") for big in (False, True) if shapes_of(rule, big)]


@pytest.mark.parametrize("rule, pattern, big", BATCHES, ids=[f"{r}-{p}-{'above' if b else 'up to'} 4M pixels" for r, p, b in BATCHES])
def test_the_extreme_shapes_are_bit_exact_in_both_packings(eng, rule, pattern, big):
    shapes = shapes_of(rule, big)
    rec = check_against_the_plan(rule, shapes)
    arrays = [image(pattern, h, w) for h, w in shapes]
    lut = opre.normalise_lut()
    try:
        if rule == "tiles560":
            got, ids, nt = run_tiles(eng, *pack(arrays, tight=False))
            bad = []
            for k, (s, a) in enumerate(zip(shapes, arrays)):
                want, aid, n_t, grid = opre.preprocess_tiles(a, 560, 4)
                assert (int(ids[k]), nt[k]) == (aid, n_t) and grid == (rec["th"][k], rec["tw"][k]) and n_t == rec["th"][k] * rec["tw"][k], (s, "grid")
                assert opre.supported_aspect_ratios(4).index((int(rec["th"][k]), int(rec["tw"][k]))) + 1 == int(ids[k]), (s, "the plan's grid")
                if not np.array_equal(got[k], want.view(np.uint32)):
                    bad.append((s, int((got[k] != want.view(np.uint32)).sum())))
            assert not bad, f"{rule} {pattern}: (shape, values that differ) {bad}"
            tight, ids_t, nt_t = run_tiles(eng, *pack(arrays, tight=True))
            assert ids_t.tolist() == ids.tolist() and nt_t == nt
        else:
            set_rule(eng, rule)
            got = run_patches(eng, *pack(arrays, tight=False))
            bad = []
            for k, (s, a) in enumerate(zip(shapes, arrays)):
                want = expected_patches(rule, a, lut)
                if not np.array_equal(got[k], want):
                    bad.append((s, int((got[k] != want).sum())))
            assert not bad, f"{rule} {pattern}: (shape, values that differ) {bad}"
            tight = run_patches(eng, *pack(arrays, tight=True))
        differ = [s for k, s in enumerate(shapes) if not np.array_equal(tight[k], got[k])]
        assert not differ, f"{rule} {pattern}: the tightly packed run differs from the aligned one at {differ}"
    finally:
        eng.set_resize_rule("fit_pad")


@pytest.mark.parametrize("rule, large", [("fit_pad", (70, 7841)), ("clip", (2000, 1990))])
def test_the_batch_maximum_of_kv_does_not_move_the_other_crops(eng, rule, large):
    """kvs, the stride of a band's coefficient rows in LDS, is the batch's largest kv: 144 here under fit-and-pad (the largest
    of the rule) and 40 under CLIP's, against 0..12 of the other crops"""
    others = [(224, 224), (1, 1), (300, 500), (500, 300), (225, 1), (113, 1), (37, 1000), (640, 480)]
    rec, tot = Engine.k1_plan(*_plan_args(rule), np.array(others + [large], dtype=np.int32))
    assert rec["kv"][-1] == tot[3] == (144 if rule == "fit_pad" else 40) and rec["kv"][:-1].max() <= 12
    arrays = [image("noise", h, w) for h, w in others]
    big = image("binary", *large)
    lut = opre.normalise_lut()
    try:
        set_rule(eng, rule)
        alone = run_patches(eng, *pack(arrays, tight=False))
        last = run_patches(eng, *pack(arrays + [big], tight=False))
        first = run_patches(eng, *pack([big] + arrays, tight=False))
        assert np.array_equal(last[:-1], alone) and np.array_equal(first[1:], alone)
        want = expected_patches(rule, big, lut)
        assert np.array_equal(last[-1], want) and np.array_equal(first[0], want)
    finally:
        eng.set_resize_rule("fit_pad")


def test_a_refused_tile_batch_names_the_crop_the_plan_flags(eng):
    shapes = [(40, 33), (20, 20), (1265, 9), (30, 30)]  # at (16, 1): 1265 rows become 16, a window of 161 taps
    rec, _ = Engine.k1_plan("tiles", np.array(shapes, dtype=np.int32), tile=16, max_tiles=1)
    assert rec["refused"].tolist() == [0, 0, 2, 0] and rec["kv"][2] == 161
    pix, offs, hw = pack([image("noise", h, w) for h, w in shapes], tight=False)
    with pytest.raises(MmeError, match=r"crop 2 is 1265x9 \(h x w\) and becomes 16 rows: a vertical window of 161 taps"):
        eng.preprocess_tiles(pix, offs, hw, 16, 1)
    got, _, _ = run_tiles(eng, *pack([image("noise", h, w) for h, w in shapes[:2]], tight=True), tile=16, max_tiles=1)  # the next call works
    for k, s in enumerate(shapes[:2]):
        assert np.array_equal(got[k], opre.preprocess_tiles(image("noise", *s), 16, 1)[0].view(np.uint32)), s
