"""K1 under MME_RESIZE_CLIP on the GPU: CLIP's shortest-edge BICUBIC resize + centre crop, against the numpy restatement
of tests/clip_preprocess_reference.py (itself pinned to Pillow and transformers by tests/test_clip_preprocess_cpu.py).

(1) mme_preprocess patches are bit-equal to patchify(bf16(normalise_lut[window])) for every case of the fixture, all shapes
    mixed in one batch, in both orders, with the fma emitter (CLIP's constants) and with the table emitter;
(2) the rule as state of a context; (3) mme_embed == mme_preprocess -> mme_vit_forward; (4) RegionEmbedder end to end against
the f32 restatement of the tower fed the restated pixels, max(1 - cos) <= 1e-3 (the project's bound for this tower), and the
rule is live: the default rule's vectors differ by more than that; (5) refusals.
What that bound cannot see on std 0.02 weights (uniform attention, Q and K exchanged, a dropped key, the other activation):
tests/test_gpu_tower_sharpness.py.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import clip_preprocess_reference as cpr  # noqa: E402
import clip_reference as cr  # noqa: E402
import make_clip_golden as mk  # noqa: E402

from multimodal_embeddings_amd._lib import Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.weights import CLIP_B16, make_clip_weights, make_vit_weights, round_to_bf16  # noqa: E402
from oracle.preprocess import CLIP_MEAN, CLIP_STD, normalise_lut, patchify  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
CASES = json.load(open(os.path.join(GOLDEN, "clip_preprocess_cases.json")))["cases"]
TABLE_SET = ((0.5908, 0.5098, 0.7532), (0.2858, 0.101, 0.6727))  # no exact fma pair for channel 1: the emitter reads the table
B2P = dataclasses.replace(CLIP_B16, num_layers=2)  # CLIP-B/16 width, 2 layers, 512-d projection
_images = {}


def image_of(case):
    if case["name"] not in _images:
        a = cpr.bundled_crop(GOLDEN, case["name"]) if case["kind"] == "bundled" else cpr.case_image(case["kind"], case["h"], case["w"], case["seed"])
        _images[case["name"]] = a
    return _images[case["name"]]


def window_of(case):
    return cpr.restated_window(case["name"], image_of(case))


def pack(arrays, device="cuda:0"):
    hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(arrays), dtype=np.int64)
    offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
    for a, o, s in zip(arrays, offs, sizes):
        buf[o : o + s] = a.reshape(-1)
    return torch.from_numpy(buf).to(device), offs, hw


def bf16_bits(x_f32: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(round_to_bf16(x_f32), dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def expected_bits(case, lut) -> np.ndarray:
    win = window_of(case)
    return bf16_bits(patchify(np.stack([lut[c][win[:, :, c]] for c in range(3)])))  # [196, 768]


def device_bits(patches) -> np.ndarray:
    return patches.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1, 196, 768)


SMALL = [c for c in CASES if c["h"] * c["w"] <= 640 * 480 and c["kind"] != "bundled"]  # the quick mixed batch of the state tests


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- (1) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["fma", "table"])
def test_patches_are_bit_equal_to_the_restatement(eng, norm):
    mean, std = (CLIP_MEAN, CLIP_STD) if norm == "fma" else TABLE_SET
    lut = normalise_lut(mean, std)
    try:
        eng.set_normalisation(mean, std)
        assert eng.normalisation_form()[0] is (norm == "fma")
        eng.set_resize_rule("clip")
        assert eng.resize_rule == "clip"
        for order in (CASES, CASES[::-1]):  # every shape mixed in ONE batch, then reversed
            pix, offs, hw = pack([image_of(c) for c in order])
            got = device_bits(eng.preprocess(pix, offs, hw))
            torch.cuda.synchronize()
            bad = []
            for i, c in enumerate(order):
                want = expected_bits(c, lut)
                if not np.array_equal(got[i], want):
                    bad.append((c["name"], int((got[i] != want).sum())))
            assert not bad, f"{norm}: {len(bad)} of {len(order)} crops differ (name, values): {bad[:8]}"
    finally:
        eng.set_normalisation(CLIP_MEAN, CLIP_STD)
        eng.set_resize_rule("fit_pad")


# ---- (2) --------------------------------------------------------------------------------------------------------------
def test_rule_is_state_of_the_context(eng):
    fresh = Engine(0)
    try:
        assert fresh.resize_rule == "fit_pad"
        pix, offs, hw = pack([image_of(c) for c in SMALL])
        never = device_bits(fresh.preprocess(pix, offs, hw))
        fresh.set_resize_rule("clip")
        under_clip = device_bits(fresh.preprocess(pix, offs, hw))
        fresh.set_resize_rule("fit_pad")
        assert fresh.resize_rule == "fit_pad"
        back = device_bits(fresh.preprocess(pix, offs, hw))
        assert np.array_equal(back, never)
        assert np.array_equal(device_bits(eng.preprocess(pix, offs, hw)), never)  # another context that never changed
        assert not np.array_equal(under_clip, never)
        # an all-224 x 224 batch is the identity under both rules
        sq = [cpr.case_image("noise", 224, 224, 50 + i) for i in range(5)]
        p2, o2, h2 = pack(sq)
        a = device_bits(fresh.preprocess(p2, o2, h2))
        fresh.set_resize_rule("clip")
        b = device_bits(fresh.preprocess(p2, o2, h2))
        assert np.array_equal(a, b)
        lut = normalise_lut()
        assert np.array_equal(b[0], bf16_bits(patchify(np.stack([lut[c][sq[0][:, :, c]] for c in range(3)]))))
        # no weight load changes the rule
        fresh.load_clip(make_clip_weights(15, B2P), geom=B2P)
        assert fresh.resize_rule == "clip"
        fresh.load_vit(make_vit_weights(seed=1))
        assert fresh.resize_rule == "clip"
        # an embedder around a caller's engine leaves the engine's rule alone and reports it
        assert RegionEmbedder(engine=fresh).resize_rule == "clip" and fresh.resize_rule == "clip"
        assert RegionEmbedder(engine=fresh, resize_rule="fit_pad").resize_rule == "fit_pad" and fresh.resize_rule == "fit_pad"
        fresh.set_resize_rule("clip")
        with pytest.raises(MmeError, match=r"rule 7; supported 0 .*1 "):
            fresh.set_resize_rule(7)
        assert fresh.resize_rule == "clip"
        with pytest.raises(MmeError, match="bicubic"):
            fresh.set_resize_rule("bicubic")
    finally:
        fresh.close()


# ---- (3) --------------------------------------------------------------------------------------------------------------
def test_embed_equals_preprocess_then_forward(eng):
    e = Engine(0)
    try:
        e.load_clip(make_clip_weights(15, B2P), geom=B2P)
        e.set_resize_rule("clip")
        pix, offs, hw = pack([image_of(c) for c in SMALL])
        a32, a16 = e.embed(pix, offs, hw)
        b32, b16 = e.vit_forward(e.preprocess(pix, offs, hw))
        torch.cuda.synchronize()
        assert torch.equal(a32.view(torch.int32), b32.view(torch.int32)) and torch.equal(a16.view(torch.int16), b16.view(torch.int16))
    finally:
        e.close()


# ---- (4) --------------------------------------------------------------------------------------------------------------
E2E = [c for c in CASES if c["h"] != c["w"]]  # the non-square seeded crops and the bundled crops (none of which is square)


@pytest.mark.parametrize("key", ["B2P", "B"])
def test_end_to_end_against_the_tower_fed_the_restated_pixels(key):
    assert sum(c["kind"] == "bundled" for c in E2E) == 24
    geom, w = (B2P, make_clip_weights(15, B2P)) if key == "B2P" else (mk.CASES["B"][1], make_clip_weights(*mk.CASES["B"]))
    arrays = [image_of(c) for c in E2E]
    lut = normalise_lut()
    pv = np.stack([np.stack([lut[ch][window_of(c)[:, :, ch]] for ch in range(3)]) for c in E2E]).astype(np.float32)
    want = cr.clip_embed(pv, w, geom, torch.float32, "cls")
    emb = RegionEmbedder(device=0, encoder="clip", weights=w, geometry=geom, pool="cls", chunk=64, resize_rule="clip")
    try:
        assert emb.resize_rule == "clip" and all(e.resize_rule == "clip" for e in emb.engines)
        pix, offs, hw = pack(arrays)
        got = emb.embed_packed(pix, offs, hw)[0].cpu().numpy()
        rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)
        assert ok.all() and np.array_equal(rows, got[:3])
    finally:
        for e in emb.engines:
            e.close()
    omc = cr.one_minus_cos(got, want)
    print(f"clip rule end to end {key}: max(1 - cos) = {omc.max():.3g} over {len(E2E)} crops")
    assert float(omc.max()) <= 1e-3, (key, float(omc.max()))
    if key != "B2P":
        return
    # the rule is live: the default rule's vectors of the same crops are another thing altogether
    dflt = RegionEmbedder(device=0, encoder="clip", weights=w, geometry=geom, pool="cls", chunk=64, resize_rule=None)
    try:
        assert dflt.resize_rule == "fit_pad" and dflt.engine.resize_rule == "fit_pad"
        other = dflt.embed_packed(pix, offs, hw)[0].cpu().numpy()
    finally:
        for e in dflt.engines:
            e.close()
    diff = cr.one_minus_cos(other, got)
    print(f"fit_pad against clip on the same crops: max(1 - cos) = {diff.max():.3g}")
    assert float(diff.max()) > 1e-3


# ---- (5) --------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    pix = torch.zeros(8001 * 10 * 3 + 16, dtype=torch.uint8, device="cuda:0")
    msgs = []
    try:
        for rule in ("fit_pad", "clip"):
            eng.set_resize_rule(rule)
            with pytest.raises(MmeError) as ei:
                eng.preprocess(pix, [0], [[8001, 10]])
            msgs.append(str(ei.value))
    finally:
        eng.set_resize_rule("fit_pad")
    assert msgs[0] == msgs[1] and "8001x10" in msgs[0] and "1..8000" in msgs[0]
    with pytest.raises(MmeError, match=r"'clip'.*'mllama_tiles'"):
        RegionEmbedder(device=0, encoder="mllama_tiles", resize_rule="clip")
