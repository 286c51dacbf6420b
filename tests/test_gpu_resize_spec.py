"""K1 under MME_RESIZE_SPEC on the GPU: the preprocessing a checkpoint's preprocessor_config.json asks for, against the numpy
restatement of tests/resize_spec_reference.py (itself pinned to Pillow and transformers by tests/test_resize_spec_cpu.py).

(1) mme_preprocess patches are bit-equal to patchify(bf16(normalise_lut[window])) for every case under each of the four specs,
    all shapes mixed in one batch and then reversed; the fma emitter under all four, the table emitter under one;
(2) the spec {shortest edge, 224, BICUBIC} gives the bits of rule "clip"; (3) the spec as state of a context, the identity
    shortcut and where it must not be taken; (4) patch-32 and patch-14 contexts; (5) mme_embed == mme_preprocess ->
    mme_vit_forward; (6) seeded ViT, SigLIP and DINOv2 towers under their own specs against the f32 references fed the
    restated pixels, max(1 - cos) <= 1e-3, and the rule is live; (7) resize_rule="checkpoint" from a directory; (8) refusals
    through the C ABI; (9) preprocess under a spec on a side stream is ordered on that stream (tests/stream_probes.py).

Measured on an MI355X, (6), max(1 - cos) over 52 crops under the tower's own spec | under the default rule against the same
reference: vit 1.82e-05 | 1.61, siglip_vit 1.14e-05 | 1.48, dinov2 3.27e-05 | 1.57 (the thin crops of the list are mostly
padding under the default rule).  The module: 24 tests in 9 s.
"""
import ctypes as C
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
import dinov2_reference as dr  # noqa: E402
import resize_spec_reference as rsr  # noqa: E402
import siglip_reference as sr  # noqa: E402
import stream_probes as sp  # noqa: E402
from test_gpu_clip_preprocess import TABLE_SET, bf16_bits, device_bits, pack  # noqa: E402
from test_vit32_cpu import retile_np  # noqa: E402

from multimodal_embeddings_amd import checkpoint as ckpt  # noqa: E402
from multimodal_embeddings_amd._lib import Engine, MmeError, ResizeSpec, _ResizeSpec  # noqa: E402
from multimodal_embeddings_amd.embedder import RegionEmbedder  # noqa: E402
from multimodal_embeddings_amd.staging import packed_layout  # noqa: E402
from multimodal_embeddings_amd.weights import (CLIP_B16, DINOV2_B14, SIGLIP_B16, VIT_B16, VIT_B32, make_clip_weights, make_dinov2_weights,  # noqa: E402
                                               make_siglip_weights, make_vit_weights)
from oracle.preprocess import CLIP_MEAN, CLIP_STD, normalise_lut, patchify  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
CASES = rsr.case_list()
SMALL = [c for c in CASES if c[2] * c[3] <= 640 * 480]  # the quick mixed batch
SPEC_KEYS = list(rsr.SPECS)
EDGE256 = rsr.SPECS["edge256_bicubic"]
MME_E_ARG, MME_E_STATE = -1, -2


def image_of(case):
    return rsr.case_image(*case)


def expected_bits(key, case, lut) -> np.ndarray:
    win = rsr.restated_window(key, case[0], image_of(case))
    return bf16_bits(patchify(np.stack([lut[c][win[:, :, c]] for c in range(3)])))  # [196, 768]


def expected_batch(key, cases, lut=None) -> np.ndarray:
    lut = normalise_lut() if lut is None else lut
    return np.stack([expected_bits(key, c, lut) for c in cases])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- (1) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key, norm", [(k, "fma") for k in SPEC_KEYS] + [("edge256_bicubic", "table")])
def test_patches_are_bit_equal_to_the_restatement(eng, key, norm):
    mean, std = (CLIP_MEAN, CLIP_STD) if norm == "fma" else TABLE_SET
    lut = normalise_lut(mean, std)
    try:
        eng.set_normalisation(mean, std)
        assert eng.normalisation_form()[0] is (norm == "fma")
        eng.set_resize_spec(rsr.SPECS[key])
        assert eng.resize_rule == "spec" and eng.resize_spec == rsr.SPECS[key]
        for order in (CASES, CASES[::-1]):  # every shape mixed in ONE batch, then reversed
            pix, offs, hw = pack([image_of(c) for c in order])
            got = device_bits(eng.preprocess(pix, offs, hw))
            torch.cuda.synchronize()
            bad = []
            for i, c in enumerate(order):
                want = expected_bits(key, c, lut)
                if not np.array_equal(got[i], want):
                    bad.append((c[0], int((got[i] != want).sum())))
            assert not bad, f"{key} {norm}: {len(bad)} of {len(order)} crops differ (name, values): {bad[:8]}"
    finally:
        eng.set_normalisation(CLIP_MEAN, CLIP_STD)
        eng.set_resize_rule("fit_pad")


# ---- (2) --------------------------------------------------------------------------------------------------------------
def test_the_spec_of_clips_rule_gives_clips_bits(eng):
    pix, offs, hw = pack([image_of(c) for c in SMALL])
    try:
        eng.set_resize_rule("clip")
        under_clip = device_bits(eng.preprocess(pix, offs, hw))
        eng.set_resize_spec("shortest_edge", 224, 3)
        assert eng.resize_rule == "spec" and eng.resize_spec == ResizeSpec("shortest_edge", 224, 0, 3)
        under_spec = device_bits(eng.preprocess(pix, offs, hw))
        torch.cuda.synchronize()
    finally:
        eng.set_resize_rule("fit_pad")
    assert np.array_equal(under_spec, under_clip)
    want = np.stack([bf16_bits(patchify(np.stack([normalise_lut()[c][cpr.clip_window_u8(image_of(k))[:, :, c]] for c in range(3)]))) for k in SMALL[:6]])
    assert np.array_equal(under_spec[:6], want)


# ---- (3) --------------------------------------------------------------------------------------------------------------
def test_spec_is_state_of_the_context(eng):
    fresh = Engine(0)
    try:
        assert fresh.resize_rule == "fit_pad" and fresh.resize_spec is None
        pix, offs, hw = pack([image_of(c) for c in SMALL])

        def run(e=fresh):
            out = device_bits(e.preprocess(pix, offs, hw))
            torch.cuda.synchronize()
            return out

        never = run()
        fresh.set_resize_spec(EDGE256)
        assert fresh.resize_rule == "spec" and fresh.resize_spec == EDGE256
        assert np.array_equal(run(), expected_batch("edge256_bicubic", SMALL))
        fresh.set_resize_rule("fit_pad")
        assert fresh.resize_rule == "fit_pad" and fresh.resize_spec is None
        assert np.array_equal(run(), never)
        fresh.set_resize_spec("exact", 224, 2)
        assert fresh.resize_spec == rsr.SPECS["exact224_bilinear"] == ResizeSpec("exact", 224, 224, 2)
        assert np.array_equal(run(), expected_batch("exact224_bilinear", SMALL))
        fresh.set_resize_rule("clip")
        assert fresh.resize_rule == "clip" and fresh.resize_spec is None
        under_clip = run()
        eng.set_resize_rule("clip")
        assert np.array_equal(run(eng), under_clip)
        eng.set_resize_rule("fit_pad")
        assert np.array_equal(run(eng), never)  # another context, which never held a spec
        assert not np.array_equal(under_clip, never)
        # an all-224 x 224 batch is the identity under exact 224 (either filter) ...
        sq = [cpr.case_image("noise", 224, 224, 70 + i) for i in range(5)]
        p2, o2, h2 = pack(sq)
        lut = normalise_lut()
        identity = np.stack([bf16_bits(patchify(np.stack([lut[c][a[:, :, c]] for c in range(3)]))) for a in sq])
        for key in ("exact224_bicubic", "exact224_bilinear"):
            fresh.set_resize_spec(rsr.SPECS[key])
            assert np.array_equal(device_bits(fresh.preprocess(p2, o2, h2)), identity)
        # ... and under shortest edge 256 it is not: resized to 256 x 256, then cropped
        fresh.set_resize_spec(EDGE256)
        got = device_bits(fresh.preprocess(p2, o2, h2))
        torch.cuda.synchronize()
        assert not np.array_equal(got, identity)
        want = np.stack([bf16_bits(patchify(np.stack([lut[c][rsr.spec_window_u8(EDGE256, a)[:, :, c]] for c in range(3)]))) for a in sq])
        assert np.array_equal(got, want)
        # 256 x 256 crops under shortest edge 256 are filtered on neither axis: a copy from offset (16, 16)
        sq256 = [cpr.case_image("noise", 256, 256, 80 + i) for i in range(3)]
        p3, o3, h3 = pack(sq256)
        got = device_bits(fresh.preprocess(p3, o3, h3))
        torch.cuda.synchronize()
        assert np.array_equal(got, np.stack([bf16_bits(patchify(np.stack([lut[c][a[16:240, 16:240, c]] for c in range(3)]))) for a in sq256]))
        # no weight load touches the spec
        geom = dataclasses.replace(CLIP_B16, num_layers=1)
        fresh.load_clip(make_clip_weights(15, geom), geom=geom)
        assert fresh.resize_rule == "spec" and fresh.resize_spec == EDGE256
        # an embedder around a caller's engine leaves the spec alone and reports it
        emb = RegionEmbedder(engine=fresh, encoder="clip")
        assert emb.resize_rule == "spec" and emb.resize_spec == EDGE256 and fresh.resize_spec == EDGE256
        emb = RegionEmbedder(engine=fresh, encoder="clip", resize_rule=rsr.SPECS["exact256_bicubic"])
        assert emb.resize_rule == "spec" and emb.resize_spec == fresh.resize_spec == rsr.SPECS["exact256_bicubic"]
        with pytest.raises(MmeError, match=r"rule 2; supported 0 .*1 .*mme_set_resize_spec"):
            fresh.set_resize_rule(2)  # a spec has parameters
        assert fresh.resize_spec == rsr.SPECS["exact256_bicubic"]
    finally:
        fresh.close()


# ---- (4) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["edge256_bicubic", "exact224_bilinear"])
def test_patch32_and_patch14_contexts_emit_the_retiled_restatement(key):
    g32 = dataclasses.replace(VIT_B32, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=64)
    g14 = dataclasses.replace(DINOV2_B14, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=64)
    pix, offs, hw = pack([image_of(c) for c in SMALL])
    want16 = expected_batch(key, SMALL).reshape(-1, 768)
    e32, e14 = Engine(0), Engine(0)
    try:
        e32.load_vit(make_vit_weights(2, g32), geom=g32)
        e14.load_dinov2(make_dinov2_weights(2, g14), geom=g14)
        assert e32.vit_geometry().patch_size == 32 and e14.vit_geometry().patch_size == 14
        for e in (e32, e14):
            e.set_resize_spec(rsr.SPECS[key])
            e.set_chunk(16)  # more than one chunk: the staging buffer is reused
        p32 = e32.preprocess(pix, offs, hw).view(torch.int16).cpu().numpy().view(np.uint16)
        p14 = e14.preprocess(pix, offs, hw).view(torch.int16).cpu().numpy().view(np.uint16)
        torch.cuda.synchronize()
    finally:
        e32.close()
        e14.close()
    assert np.array_equal(p32, retile_np(want16.view(np.int16)).view(np.uint16))
    assert np.array_equal(p14, dr.retile_p14_reference(want16.view(np.int16)).view(np.uint16))


# ---- (5) --------------------------------------------------------------------------------------------------------------
def test_embed_equals_preprocess_then_forward():
    geom = dataclasses.replace(SIGLIP_B16, num_layers=2)
    e = Engine(0)
    try:
        e.load_siglip(make_siglip_weights(4, geom), geom=geom)
        e.set_resize_spec(rsr.SPECS["exact224_bicubic"])
        pix, offs, hw = pack([image_of(c) for c in SMALL])
        a32, a16 = e.embed(pix, offs, hw)
        b32, b16 = e.vit_forward(e.preprocess(pix, offs, hw))
        torch.cuda.synchronize()
        assert torch.equal(a32.view(torch.int32), b32.view(torch.int32)) and torch.equal(a16.view(torch.int16), b16.view(torch.int16))
    finally:
        e.close()


# ---- (6) --------------------------------------------------------------------------------------------------------------
def e2e_crops():
    """The non-square small cases and the 24 bundled crops: (name, image)."""
    crops = [(c[0], image_of(c)) for c in SMALL if c[2] != c[3]]
    names = sorted(f for f in os.listdir(os.path.join(GOLDEN, "crops")) if f.endswith(".png"))
    assert len(names) == 24
    return crops + [(n, cpr.bundled_crop(GOLDEN, n)) for n in names]


def _vit_want(pv, w, geom):
    from oracle import vit as ovit

    return ovit.vit_embed(np.stack([patchify(p) for p in pv]), w, geom, pool="cls")


TOWERS = {
    "vit": ("exact224_bilinear", dataclasses.replace(VIT_B16, num_layers=2), lambda g: make_vit_weights(3, g), _vit_want),
    "siglip_vit": ("exact224_bicubic", dataclasses.replace(SIGLIP_B16, num_layers=2), lambda g: make_siglip_weights(4, g),
                   lambda pv, w, g: sr.siglip_embed(pv, w, g, torch.float32)),
    "dinov2": ("edge256_bicubic", dataclasses.replace(DINOV2_B14, num_layers=2), lambda g: make_dinov2_weights(6, g),
               lambda pv, w, g: dr.dinov2_embed(pv, w, g, torch.float32)),
}


@pytest.mark.parametrize("encoder", list(TOWERS))
def test_end_to_end_against_the_tower_fed_the_restated_pixels(encoder):
    key, geom, make, reference = TOWERS[encoder]
    spec = rsr.SPECS[key]
    w = make(geom)
    crops = e2e_crops()
    arrays = [a for _, a in crops]
    lut = normalise_lut()
    pv = np.stack([np.stack([lut[ch][rsr.restated_window(key, name, a)[:, :, ch]] for ch in range(3)]) for name, a in crops]).astype(np.float32)
    want = reference(pv, w, geom)
    pix, offs, hw = pack(arrays)
    got = {}
    for rule in (spec, None):
        emb = RegionEmbedder(device=0, encoder=encoder, weights=w, geometry=geom, chunk=64, resize_rule=rule)
        try:
            if rule is None:
                assert emb.resize_rule == "fit_pad" and emb.resize_spec is None
            else:
                assert emb.resize_rule == "spec" and emb.resize_spec == spec and all(e.resize_spec == spec for e in emb.engines)
            got[rule] = emb.embed_packed(pix, offs, hw)[0].cpu().numpy()
            if rule is not None:
                rows, ok = emb.get_image_embeddings(arrays[:3], as_array=True)
                assert ok.all() and np.array_equal(rows, got[rule][:3])
        finally:
            for e in emb.engines:
                e.close()
    omc = sr.one_minus_cos(got[spec], want)
    other = sr.one_minus_cos(got[None], want)
    print(f"{encoder} under {spec}: max(1 - cos) = {omc.max():.3g} over {len(crops)} crops; under the default rule {other.max():.3g}")
    assert float(omc.max()) <= 1e-3, (encoder, float(omc.max()))
    assert float(other.max()) > 1e-3, (encoder, float(other.max()))  # the rule is live


# ---- (7) --------------------------------------------------------------------------------------------------------------
DINOV2_PC = {"image_processor_type": "BitImageProcessor", "do_resize": True, "size": {"shortest_edge": 256}, "resample": 3, "do_center_crop": True,
             "crop_size": {"height": 224, "width": 224}, "do_rescale": True, "rescale_factor": 1.0 / 255.0, "do_normalize": True, "do_convert_rgb": True,
             "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225]}


def test_rule_from_a_directory(tmp_path):
    geom = dataclasses.replace(DINOV2_B14, hidden_size=384, num_heads=6, num_layers=1, intermediate_size=64)
    d = ckpt.save_checkpoint(tmp_path / "dinov2", make_dinov2_weights(2, geom), "dinov2", "float32", geometry=geom, image_mean=DINOV2_PC["image_mean"],
                             image_std=DINOV2_PC["image_std"])
    with open(os.path.join(d, "preprocessor_config.json"), "w") as fh:
        json.dump(DINOV2_PC, fh)
    pix, offs, hw = pack([image_of(c) for c in SMALL])
    rows = {}
    for rule in ("checkpoint", EDGE256):
        emb = RegionEmbedder(d, device=0, encoder="dinov2", resize_rule=rule, chunk=64)
        try:
            assert emb.engine.resize_spec == EDGE256 and emb.engine.resize_rule == "spec" and emb.resize_spec == EDGE256
            assert emb.checkpoint.resize_spec == (EDGE256 if rule == "checkpoint" else None)
            rows[rule] = emb.embed_packed(pix, offs, hw)[0].cpu()
        finally:
            for e in emb.engines:
                e.close()
    assert torch.equal(rows["checkpoint"].view(torch.int32), rows[EDGE256].view(torch.int32))
    with open(os.path.join(d, "preprocessor_config.json"), "w") as fh:
        json.dump({**DINOV2_PC, "resample": 1}, fh)
    os.rename(os.path.join(d, "model.safetensors"), os.path.join(d, "model.safetensors.away"))  # nothing is loaded before the refusal
    with pytest.raises(MmeError, match=r"preprocessor_config\.json: resample = 1; supported 2 \(Pillow BILINEAR\) and 3 \(Pillow BICUBIC\)"):
        RegionEmbedder(d, device=0, encoder="dinov2", resize_rule="checkpoint")


# ---- (8) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw, match", [
    ((0, 223, 0, 3), r"height = 223 \(the shortest edge\); supported 224\.\.512"),
    ((0, 513, 0, 3), r"height = 513 \(the shortest edge\); supported 224\.\.512"),
    ((1, 224, 513, 3), r"width = 513; supported 224\.\.512"),
    ((1, 223, 224, 2), r"height = 223 \(the height of the resized image\); supported 224\.\.512"),
    ((0, 256, 256, 3), r"width = 256; supported 0 under MME_RESIZE_MODE_SHORTEST_EDGE"),
    ((0, 256, 0, 1), r"resample = 1; supported 2 \(Pillow BILINEAR\) and 3 \(Pillow BICUBIC\)"),
    ((7, 256, 0, 3), r"mode = 7; supported 0 \(MME_RESIZE_MODE_SHORTEST_EDGE\) and 1 \(MME_RESIZE_MODE_EXACT\)"),
], ids=["edge_223", "edge_513", "width_513", "height_223", "width_with_an_edge", "resample_1", "mode_7"])
def test_refusals_through_the_c_abi(eng, raw, match):
    import re

    lib, h = eng.lib, eng.h
    pix, offs, hw = pack([image_of(c) for c in SMALL[:6]])
    for before in (None, rsr.SPECS["exact256_bicubic"]):  # from the default rule and from a spec: the rule stays what it was
        if before is None:
            eng.set_resize_rule("fit_pad")
        else:
            eng.set_resize_spec(before)
        try:
            bits = device_bits(eng.preprocess(pix, offs, hw))
            assert lib.mme_set_resize_spec(h, C.byref(_ResizeSpec(*raw))) == MME_E_ARG
            msg = lib.mme_last_error(h).decode()
            assert re.search(match, msg) and msg.startswith("mme_set_resize_spec: "), msg
            with pytest.raises(MmeError, match=match):
                eng.set_resize_spec(ResizeSpec(raw[0], *raw[1:]))
            assert eng.resize_spec == before and eng.resize_rule == ("fit_pad" if before is None else "spec")
            assert np.array_equal(device_bits(eng.preprocess(pix, offs, hw)), bits)
        finally:
            eng.set_resize_rule("fit_pad")


def test_null_pointers_and_reading_a_spec_that_is_not_the_rule(eng):
    lib, h = eng.lib, eng.h
    out = _ResizeSpec(-5, -5, -5, -5)
    eng.set_resize_rule("clip")
    try:
        assert lib.mme_get_resize_spec(h, C.byref(out)) == MME_E_STATE
        msg = lib.mme_last_error(h).decode()
        assert "the current rule is 1, not 2 (MME_RESIZE_SPEC)" in msg and "mme_set_resize_spec" in msg
        assert (out.mode, out.height, out.width, out.resample) == (-5, -5, -5, -5)
        assert lib.mme_set_resize_spec(h, None) == MME_E_ARG and "spec is NULL" in lib.mme_last_error(h).decode()
        assert lib.mme_get_resize_spec(h, None) == MME_E_ARG and "null argument" in lib.mme_last_error(h).decode()
        assert lib.mme_set_resize_spec(None, C.byref(_ResizeSpec(0, 256, 0, 3))) == MME_E_ARG
        assert lib.mme_get_resize_spec(None, C.byref(out)) == MME_E_ARG
        assert eng.resize_rule == "clip" and eng.resize_spec is None
        assert lib.mme_set_resize_spec(h, C.byref(_ResizeSpec(1, 512, 224, 2))) == 0
        assert lib.mme_get_resize_spec(h, C.byref(out)) == 0 and (out.mode, out.height, out.width, out.resample) == (1, 512, 224, 2)
        # crops stay 1..8000 per side under a spec, with the message of the other rules
        big = torch.zeros(8001 * 10 * 3 + 16, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(MmeError, match=r"8001x10.*1\.\.8000"):
            eng.preprocess(big, [0], [[8001, 10]])
    finally:
        eng.set_resize_rule("fit_pad")
    with pytest.raises(MmeError, match=r"'mllama_tiles'"):
        RegionEmbedder(device=0, encoder="mllama_tiles", resize_rule=EDGE256)


# ---- (9) --------------------------------------------------------------------------------------------------------------
STREAM_HW = np.array([[224, 224], [37, 300], [300, 41]], dtype=np.int32)  # (h, w): resized and cropped, a wide and a tall crop


def stream_crops(v):
    """Three packed crops.  The overwrite (v = 2) of the host tables: every crop 8 x 8 at offset 0, so that any mixture of old
    and new offsets and sizes stays inside the packed buffer."""
    offs, sizes, total = packed_layout(STREAM_HW)
    rng = np.random.default_rng(300 + v)
    pix = np.zeros(total, dtype=np.uint8)
    for o, n in zip(offs, sizes):
        pix[o:o + n] = rng.integers(0, 256, int(n), dtype=np.uint8)
    if v == 2:
        return {"pix": torch.from_numpy(pix)}, {"offs": np.zeros(3, dtype=np.int64), "hw": np.full((3, 2), 8, dtype=np.int32)}
    return {"pix": torch.from_numpy(pix)}, {"offs": offs.astype(np.int64), "hw": STREAM_HW.copy()}


def spec_engine():
    e = Engine(0)
    e.set_resize_spec(EDGE256)
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("probe", ["A", "B"])
def test_preprocess_under_a_spec_runs_on_the_callers_stream(probe):
    case = sp.Case("preprocess", "preprocess-spec-edge256", spec_engine, stream_crops,
                   lambda e, d, h: {"patches": e.preprocess(d["pix"], h["offs"], h["hw"])})
    # the reference of the probes is the same call on the default stream; it is itself the restatement
    dev, host = stream_crops(0)
    lut = normalise_lut()
    want = np.stack([bf16_bits(patchify(np.stack([lut[c][rsr.spec_window_u8(EDGE256, dev["pix"].numpy()[o:o + h * w * 3].reshape(h, w, 3))[:, :, c]]
                                                  for c in range(3)]))) for o, (h, w) in zip(host["offs"], host["hw"])])
    assert np.array_equal(sp.reference(case, 0)["patches"].view(np.uint16).reshape(3, 196, 768), want)
    bad, effective = (sp.probe_a if probe == "A" else sp.probe_b)(case)
    print(f"preprocess under a spec, probe {probe}: effective = {effective}")
    assert not bad, bad
