"""The sharp weights of tests/tower_mutants.py tell a wrong tower from a right one; no GPU.

Per case (two layers; three crops, or eight token sequences of different lengths), on the float64 restatements:
  (a) the restatement's bf16 emulation (float32 arithmetic, values rounded to bf16 where the engine stores bf16: the patch
      matrix, x behind the embedding and behind each residual add, q | k | v, the attention output, the activation output)
      is within 2.5e-4 of float64 on every crop or sequence: a quarter of the project's bound, a condition on the INPUTS that
      makes the GPU assertion of tests/test_gpu_tower_sharpness.py reachable, no tolerance for the engine;
  (b) every required mutant is at least 4e-3 from the restatement on at least half of the crops or sequences (the metric:
      per crop the maximum of 1 - cos over every row of every output the GPU test compares);
  (c) the same mutants on `make_*_weights(std=0.02)`, the weights of every other end-to-end test, are printed beside it
      (`pytest -s`), not asserted.

One mutant is recorded and not asserted, RECORDED_ONLY of tests/tower_mutants.py: tanh-GELU against erf-GELU in the towers that
run one of the two (ViT, DINOv2, SigLIP image and text).  With the pre-activations moved to -2.5 +- 1 it measures 2e-5 to 1e-4;
fc1.bias - 3.0 gives 1e-4 with the emulation at 7e-4, fc1.bias - 3.5 with fc2.weight x 30 gives 4e-4 with the emulation at
6e-4 (ViT-B/16): the two forms differ by 4.7e-4 absolute at most, which a residual stream does not carry.  The kernels'
own tests hold them apart element by element: tests/test_gpu_gemm.py::test_gelu_dense_grid_fast_and_slow_path (mutant
"tanh-GELU") and tests/test_gpu_siglip.py::test_tanh_gelu_dense_grid_and_the_tails (mutant "erf-GELU").

What the text towers' zeros mean: a one-token CLIP sequence pools position 0, where attention has one key, and a full-length
sequence has its EOS at the last position; a full-length SigLIP sequence has no padding.  Those sequences cannot see the
mutants in question, the other seven can.

Measured, the value that at least half of the crops or sequences reach, sharp weights | std 0.02 ("-": not a mutant of that tower):

    sharp weights                                         ViT-B/16    ViT-B/32     ViT 384    DINOv2-B DINOv2 1024   CLIP-B/16   CLIP-B/32    SigLIP-B   CLIP text SigLIP text
    bf16 emulation (the maximum)                            6.7e-5      4.5e-5      8.2e-5      1.7e-5      6.2e-5      3.1e-5      5.0e-5      4.0e-5      8.4e-6      1.5e-5
    uniform attention                                       3.5e-1      4.5e-1      3.7e-1      1.5e-1      3.0e-1      1.6e-1      2.0e-1      2.2e-1      4.3e-2      1.7e-1
    Q and K exchanged                                       5.4e-1      7.0e-1      6.0e-1      2.6e-1      5.2e-1      2.6e-1      3.4e-1      3.7e-1      7.3e-2      2.6e-1
    no dh^-0.5                                              4.1e-1      2.3e-1      3.3e-1      4.8e-1      5.1e-1      2.7e-1      2.1e-1      3.0e-1      2.2e-1      3.2e-1
    heads rolled by one between P and V                     8.8e-1      9.5e-1      8.0e-1      7.3e-1      9.2e-1      5.6e-1      6.2e-1      5.3e-1      5.6e-1      8.1e-1
    last key dropped                                        7.0e-2      2.9e-2      2.2e-2      1.0e-2      3.6e-2      3.5e-2      3.2e-2      1.9e-2           -           -
    first key (class row) dropped                           7.4e-2      3.6e-2      5.0e-2      1.8e-2      5.1e-2      2.9e-2      5.6e-2      2.8e-2           -           -
    position rows rolled by one                             4.3e-1      4.9e-1      4.3e-1      1.1e-1      3.5e-1      2.8e-1      2.6e-1      2.2e-1      8.4e-2      2.3e-1
    class row without its position                          3.1e-1      3.2e-1      2.9e-1      1.1e-1      3.3e-1      1.8e-1      1.8e-1      4.4e-2           -           -
    ln1 / ln2 parameters exchanged                          1.8e-1      1.8e-1      2.9e-1      2.2e-1      3.8e-1      1.7e-1      2.1e-1      2.4e-1      7.6e-2      1.8e-1
    final LayerNorm left out                                6.5e-3      6.1e-3      1.0e-2      4.2e-2      4.1e-2      4.4e-2      3.4e-2      1.9e-1      3.8e-2      3.7e-2
    the neighbouring token pooled                           8.1e-1      9.5e-1      9.8e-1      6.3e-1      7.2e-1      4.2e-1      4.7e-1      7.9e-1           -           -
    residual around the MLP dropped                         8.3e-1      9.5e-1      9.4e-1      8.2e-1      9.2e-1      6.5e-1      6.8e-1      8.6e-1      4.8e-1      6.9e-1
    tanh-GELU against erf-GELU                              5.5e-5      3.3e-5      6.5e-5      7.2e-5      2.2e-5           -           -      6.6e-5           -      4.7e-5
    patch columns in (ky, kx, c) order                           -      9.7e-1           -           -           -           -      5.3e-1           -           -           -
    LayerScale left out                                          -           -           -      8.3e-2      9.5e-2           -           -           -           -           -
    ls1 / ls2 exchanged                                          -           -           -      1.5e-1      1.7e-1           -           -           -           -           -
    the class position row taken from the interpolated           -           -           -      1.3e-1      3.8e-1           -           -           -           -           -
    pre_layrnorm left out                                        -           -           -           -           -      1.7e-1      3.0e-1           -           -           -
    erf-GELU for QuickGELU                                       -           -           -           -           -      7.1e-2      6.5e-2           -      5.6e-2           -
    projection applied before post_layernorm                     -           -           -           -           -      8.3e-2      6.2e-2           -           -           -
    probe query unscaled                                         -           -           -           -           -           -           -      2.1e-1           -           -
    the head's MLP residual dropped                              -           -           -           -           -           -           -      5.0e-1           -           -
    post_layernorm left out of the K | V input                   -           -           -           -           -           -           -      1.9e-1           -           -
    mean pooling for the head                                    -           -           -           -           -           -           -      4.2e-2           -           -
    causal mask dropped                                          -           -           -           -           -           -           -           -      1.7e-1           -
    pooled at the last position for the EOS position             -           -           -           -           -           -           -           -      9.7e-2           -
    pooled one before EOS                                        -           -           -           -           -           -           -           -      7.7e-2           -
    padding masked out                                           -           -           -           -           -           -           -           -           -      2.3e-1
    position 62 pooled for 63                                    -           -           -           -           -           -           -           -           -      1.4e-1
    the head's bias left out                                     -           -           -           -           -           -           -           -           -      1.0e-2

    std 0.02                                              ViT-B/16    ViT-B/32     ViT 384    DINOv2-B DINOv2 1024   CLIP-B/16   CLIP-B/32    SigLIP-B   CLIP text SigLIP text
    bf16 emulation (the maximum)                            1.1e-5      1.2e-5      1.2e-5      1.2e-5      1.0e-5      1.3e-5      1.3e-5      1.1e-5      1.4e-5      8.9e-6
    uniform attention                                       5.6e-3      1.4e-2      8.1e-4      5.7e-3      1.1e-2      9.9e-5      2.6e-4      2.3e-4      5.6e-3      6.4e-3
    Q and K exchanged                                       1.1e-2      2.5e-2      1.5e-3      1.1e-2      2.3e-2      2.0e-4      4.6e-4      4.7e-4      1.4e-2      1.1e-2
    no dh^-0.5                                              3.9e-1      4.2e-1      5.5e-2      3.8e-1      5.0e-1      2.1e-2      2.7e-2      5.2e-2      2.6e-1      3.9e-1
    heads rolled by one between P and V                     6.5e-1      7.2e-1      4.9e-1      7.4e-1      7.8e-1      1.5e-2      1.5e-2      2.1e-1      6.7e-1      7.5e-1
    last key dropped                                        2.6e-4      3.6e-3      1.1e-4      1.4e-4      1.7e-4      4.0e-6      4.8e-5      3.6e-5           -           -
    first key (class row) dropped                           2.6e-4      3.3e-3      1.1e-4      1.9e-4      1.3e-4      4.2e-6      6.7e-5      3.8e-5           -           -
    position rows rolled by one                             6.9e-2      8.0e-2      1.4e-1      4.0e-2      3.3e-2      5.0e-1      5.1e-1      1.4e-3      1.5e-1      2.2e-2
    class row without its position                          4.1e-2      4.5e-2      9.2e-2      2.9e-2      2.1e-2      3.2e-1      2.8e-1      4.4e-4           -           -
    ln1 / ln2 parameters exchanged                          7.8e-3      7.0e-3      4.3e-3      2.5e-1      3.3e-1      2.4e-2      2.2e-2      9.2e-2      2.9e-1      1.9e-1
    final LayerNorm left out                                5.3e-3      4.6e-3      1.2e-2      4.4e-2      4.3e-2      4.3e-2      3.7e-2      7.1e-2      3.9e-2      3.7e-2
    the neighbouring token pooled                            1.1e0       1.0e0       1.1e0       1.1e0      9.8e-1       1.1e0       1.0e0       1.0e0           -           -
    residual around the MLP dropped                         8.6e-1       1.0e0       1.1e0      8.2e-1      8.9e-1      9.8e-1      9.5e-1      8.5e-1      3.8e-1      5.4e-1
    tanh-GELU against erf-GELU                              2.0e-8      2.0e-8      1.0e-8      2.1e-8      2.2e-8           -           -      2.9e-8           -      2.0e-8
    patch columns in (ky, kx, c) order                           -       1.0e0           -           -           -           -       1.1e0           -           -           -
    LayerScale left out                                          -           -           -      1.0e-1      9.9e-2           -           -           -           -           -
    ls1 / ls2 exchanged                                          -           -           -      1.9e-1      1.9e-1           -           -           -           -           -
    the class position row taken from the interpolated           -           -           -      4.6e-2      4.0e-2           -           -           -           -           -
    pre_layrnorm left out                                        -           -           -           -           -      7.8e-1      7.5e-1           -           -           -
    erf-GELU for QuickGELU                                       -           -           -           -           -      1.8e-5      1.7e-5           -      9.1e-5           -
    projection applied before post_layernorm                     -           -           -           -           -      7.5e-2      6.2e-2           -           -           -
    probe query unscaled                                         -           -           -           -           -           -           -      2.5e-1           -           -
    the head's MLP residual dropped                              -           -           -           -           -           -           -      5.2e-2           -           -
    post_layernorm left out of the K | V input                   -           -           -           -           -           -           -      7.1e-2           -           -
    mean pooling for the head                                    -           -           -           -           -           -           -      2.3e-3           -           -
    causal mask dropped                                          -           -           -           -           -           -           -           -      6.3e-1           -
    pooled at the last position for the EOS position             -           -           -           -           -           -           -           -      5.1e-1           -
    pooled one before EOS                                        -           -           -           -           -           -           -           -      2.0e-1           -
    padding masked out                                           -           -           -           -           -           -           -           -           -      5.0e-1
    position 62 pooled for 63                                    -           -           -           -           -           -           -           -           -      2.1e-2
    the head's bias left out                                     -           -           -           -           -           -           -           -           -      6.4e-4
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tower_mutants as tm  # noqa: E402


def half_value(d: np.ndarray) -> float:
    """The largest v such that at least half of the entries of d are >= v"""
    return float(np.sort(d)[::-1][math.ceil(len(d) / 2) - 1])


def sweep(key: str, sharp: bool) -> dict:
    """label -> distance per crop or sequence [n], for the emulation ("bf16 emulation"), every required mutant and the
    recorded one; the float64 reference is computed once"""
    t = tm.TOWERS[key]
    x = tm.inputs_of(key)
    x = x if t.text else x[1]
    w = tm.weights_of(key, sharp)
    ref = tm.outputs(key, w, x)
    out = {"bf16 emulation": tm.distance(tm.outputs(key, w, x, torch.float32, "bf16"), ref)}
    for label, name in {**tm.mutants_of(key), **tm.recorded_only_of(key)}.items():
        out[label] = tm.distance(tm.outputs(key, w, x, mutant=name), ref)
    return out


@pytest.mark.parametrize("key", list(tm.TOWERS))
def test_sharp_weights_separate_every_required_mutant(key):
    sharp, old = sweep(key, True), sweep(key, False)
    n = len(sharp["bf16 emulation"])
    assert n <= (tm.N_SEQ if tm.TOWERS[key].text else tm.N_CROPS)
    print(f"\n{key}: distance that at least half of the {n} items reach (min .. max), sharp weights | std 0.02")
    for label in sharp:
        print(f"  {label:58s} {half_value(sharp[label]):9.2e} ({sharp[label].min():.1e} .. {sharp[label].max():.1e}) | "
              f"{half_value(old[label]):9.2e} ({old[label].min():.1e} .. {old[label].max():.1e})")
    assert sharp["bf16 emulation"].max() <= tm.EMULATION_NEAR, (key, sharp["bf16 emulation"])
    for label in tm.mutants_of(key):
        assert half_value(sharp[label]) >= tm.MUTANT_FAR, (key, label, np.sort(sharp[label]))
    unseen = [label for label in tm.mutants_of(key) if half_value(old[label]) < tm.BOUND]
    print(f"  within the 1e-3 bound at std 0.02: {', '.join(unseen) or 'none'}")


def test_the_required_mutants_are_registered_and_one_is_recorded_only():
    image = {"uniform attention", "Q and K exchanged", "no dh^-0.5", "heads rolled by one between P and V", "last key dropped",
             "first key (class row) dropped", "position rows rolled by one", "class row without its position",
             "ln1 / ln2 parameters exchanged", "final LayerNorm left out", "the neighbouring token pooled", "residual around the MLP dropped"}
    need = {"vit": image,
            "clip": image | {"pre_layrnorm left out", "erf-GELU for QuickGELU", "projection applied before post_layernorm"},
            "dinov2": image | {"LayerScale left out", "ls1 / ls2 exchanged", "the class position row taken from the interpolated grid"},
            "siglip": image | {"probe query unscaled", "the head's MLP residual dropped", "post_layernorm left out of the K | V input",
                               "mean pooling for the head"},
            "clip_text": {"causal mask dropped", "pooled at the last position for the EOS position", "pooled one before EOS"},
            "siglip_text": {"padding masked out", "position 62 pooled for 63", "the head's bias left out"}}
    assert {t.kind for t in tm.TOWERS.values()} == set(need)
    for key, t in tm.TOWERS.items():
        have = set(tm.mutants_of(key))
        assert need[t.kind] <= have, (key, need[t.kind] - have)
        assert ("patch columns in (ky, kx, c) order" in have) == (getattr(t.geom, "patch_size", 16) == 32), key
        assert set(tm.recorded_only_of(key)) <= {"tanh-GELU against erf-GELU"} and not set(tm.recorded_only_of(key)) & have
    geoms = [t.geom for t in tm.TOWERS.values() if t.kind in ("vit", "dinov2")]
    assert sorted(g.hidden_size for g in geoms).count(384) == 1 and sorted(g.hidden_size for g in geoms).count(1024) == 1
    assert {16, 32} <= {g.patch_size for g in geoms} and all(getattr(t.geom, "num_layers") == 2 for t in tm.TOWERS.values())


def test_token_rows_are_the_final_layernorm_rows_of_the_restatements():
    """The `*_token_rows` functions (what Engine.vit_tokens returns) on one crop, float64: unit rows, equal to the rows the
    sweep compares, and row t is the tower's pooled row of token t, normalised (to float64 rounding: the same LayerNorm on
    one row or on all)."""
    import clip_reference as cr
    import dinov2_reference as dr
    import siglip_reference as sr
    import vit_reference as vr

    from multimodal_embeddings_amd import weights as W

    small = dict(hidden_size=384, num_layers=1, num_heads=6, intermediate_size=64)  # one narrow layer: the tail is what is looked at
    cases = [(W.ViTGeometry(patch_size=32, **small), W.make_vit_weights, vr.vit_token_rows, vr.vit_hidden_states, vr._final_ln,
              lambda *a: vr.vit_forward(*a, token=7)),
             (W.CLIPGeometry(**small, projection_dim=None), W.make_clip_weights, cr.clip_token_rows, cr.clip_hidden_states, cr._post_ln,
              lambda *a: cr.clip_forward(*a, tok=7)[0]),
             (W.SiglipGeometry(**small), W.make_siglip_weights, sr.siglip_token_rows, sr.siglip_hidden_states, sr._post_ln, None),
             (W.Dinov2Geometry(**small), W.make_dinov2_weights, dr.dinov2_token_rows, dr.dinov2_hidden_states, dr._final_ln,
              lambda *a: dr.dinov2_forward(*a, token=7))]
    pv = tm.inputs_of("vit_s16")[1][:1]
    for geom, make, token_rows, hidden, final_ln, pooled in cases:
        w = make(31, geom, std=0.05)
        rows = token_rows(pv, w, geom)
        assert rows.shape == (1, geom.seq_len, geom.hidden_size) and rows.dtype == np.float64
        assert np.abs(np.linalg.norm(rows, axis=2) - 1.0).max() <= 1e-12
        want = cr.final_rows(hidden(pv, w, geom, torch.float64), *final_ln(w, torch.float64), geom.layer_norm_eps).numpy()
        assert np.array_equal(rows, want), type(geom).__name__
        assert tm.one_minus_cos(rows[:, 1:], rows[:, :-1]).min() > 1e-3, "neighbouring rows differ"
        if pooled is not None:
            e = pooled(pv, w, geom, torch.float64)
            assert np.abs(e / np.linalg.norm(e, axis=1, keepdims=True) - rows[:, 7]).max() <= 1e-12, type(geom).__name__


def test_vit_reference_is_the_oracle_bit_for_bit():
    """tests/vit_reference.py with mutant=None against oracle/vit.py (what tests/test_oracle_pins.py pins to transformers), in
    float32 at the three ViT cases on one crop: the sharp weights, and at hidden 384 the std 0.02 ones as well"""
    import vit_reference as vr
    from oracle import vit as ovit
    from oracle.preprocess import patchify

    for key in ("vit_b16", "vit_b32", "vit_s16"):
        geom = tm.geom_of(key)
        pv = tm.inputs_of(key)[1][:1]
        patches = torch.from_numpy(np.stack([patchify(p, geom.patch_size) for p in pv]))
        for sharp in ((True, False) if key == "vit_s16" else (True,)):
            w = tm.weights_of(key, sharp)
            want = ovit.vit_hidden_states(patches, w, geom, final_ln=False)
            got = vr.vit_hidden_states(pv, w, geom, torch.float32)
            assert torch.equal(got, want), (key, sharp)
            for pool, tok in (("cls", 0), ("last", geom.seq_len - 1)):  # the pooled row: the same LayerNorm on one row, to float32 rounding
                e = vr.vit_forward(pv, w, geom, torch.float32, tok)
                assert np.abs(e / np.linalg.norm(e, axis=1, keepdims=True) - ovit.vit_embed(patches.numpy(), w, geom, pool)).max() <= 1e-6, (key, pool)
