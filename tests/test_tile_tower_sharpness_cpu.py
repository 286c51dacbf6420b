"""The sharp weights of the tile case (tests/tower_mutants.py: TILE_*) tell a wrong tile tower from a right one; no GPU.

The tower: 1 local + 1 gated global layer with the state behind the local layer as the intermediate feature, on three images of
1, 2 and 4 tiles (aspect-ratio ids 1, 2 and 6) from the oracle's tile preprocessing.  The metric, per image: the maximum of
1 - cos over every row of all four tiles (padding tiles included) of the final-state slice, the intermediate slice and the pooled
vector, in float64.

  (a) tests/tile_reference.py in float32 with mutant=None is oracle/mllama_vision.py bit for bit (the 2-tile image);
  (b) on all three images the float32 restatement is within EMULATION_NEAR / 10 = 2.5e-5 of the float64 one, and its bf16
      emulation (values rounded where the engine stores bf16; the points are listed in tests/tile_reference.py) within
      EMULATION_NEAR = 2.5e-4: conditions on the INPUTS that make the assertion of tests/test_gpu_tile_tower_sharpness.py (the
      engine within 1e-3 of the float32 restatement) reachable, no tolerance for the engine;
  (c) on the 2-tile image every required mutant is at least MUTANT_FAR = 4e-3 from the float32 restatement.  The 2-tile image
      because of the mask mutants: it has padding TILES (two of them: 3216 padding keys, against 28 on the 4-tile image), so
      "padding keys masked for every query", "(padding, padding) mask dropped" and "each tile attends only itself" move whole
      tiles of keys, and it has a real tile 1 for "the class row of tile 1 pooled for tile 0";
  (d) the required labels are registered.

The mutants that leave the stem and the local layer alone (tile_reference.LOCAL_FREE) start from the restatement's saved state
behind them.  The module takes 3 min 20 s on 8 threads (a forward is 5 s in float32, 15 to 20 s in float64).

Measured on the 2-tile image, the maximum of 1 - cos over all outputs against the float32 restatement (the emulation: against
float64); the second column is the same seed without the recipe, the weights of tests/test_gpu_tilevit.py, and comes from
`python tests/test_tile_tower_sharpness_cpu.py` (5 min), not from the suite:

    the 2-tile image, max(1 - cos) over all outputs           sharp weights  make_tile_vit_weights
    bf16 emulation, from float64                                    1.3e-04                1.4e-05
    uniform attention                                               1.4e-01                9.7e-03
    Q and K exchanged                                               1.8e-01                2.1e-02
    no dh^-0.5                                                      6.4e-02                1.1e-01
    heads rolled by one between P and V                             2.3e-01                8.2e-02
    padding keys masked for every query                             1.3e-01                1.2e-02
    (padding, padding) mask dropped                                 1.3e-01                1.2e-02
    each tile attends only itself                                   1.6e-01                2.6e-02
    global gates ignored                                            1.0e-02                1.9e-02
    gate used without its tanh                                      1.8e-02                3.0e-03
    gate_attn / gate_ffn exchanged                                  3.5e-02                1.1e-16
    pre-tile embedding added to the class row too                   5.4e-02                2.9e-02
    (1 - tanh g) factor dropped                                     1.6e-01                8.0e-02
    tile-embedding rows rolled by one tile                          4.7e-01                4.0e-01
    post-tile embedding left out                                    1.1e-01                4.8e-05
    post-tile embedding added before layernorm_post                 3.5e-02                1.8e-06
    layernorm_pre left out                                          6.3e-01                8.7e-01
    layernorm_post left out                                         2.5e-01                4.2e-03
    ln1 / ln2 parameters exchanged                                  8.0e-02                6.9e-04
    residual around the MLP dropped                                 1.1e+00                8.9e-01
    the class row of tile 1 pooled for tile 0                       2.1e-01                1.1e-01
    a tile's 7 padding tokens taken as real                         4.1e-03                4.3e-06
    one key of 6432 dropped                                         7.4e-03                9.7e-08
    tanh-GELU for erf-GELU (recorded only)                          2.7e-05                1.1e-08

Inside the 1e-3 bound at make_tile_vit_weights, so invisible to the tile tests there: gate_attn / gate_ffn exchanged (the
same tower: both gates are pi / 4), post-tile embedding left out, post-tile embedding added before layernorm_post, ln1 / ln2
parameters exchanged, a tile's 7 padding tokens taken as real, one key of 6432 dropped.  All outputs count here, the rows of
the padding tiles included, which is where the mask mutants show at those weights.  Per image, float32 | the bf16 emulation from float64 on the sharp weights: 1 tile 8.6e-12 | 8.5e-5,
2 tiles 1.0e-11 | 1.3e-4, 4 tiles 1.1e-11 | 9.3e-5.

The narrowest required mutant is "a tile's 7 padding tokens taken as real" at 4.1e-3: it changes what 14 padding queries of the
local layer see, and reaches a real row only through those 14 rows as keys of the global layer.  It is what fixes the q / k
factor at 4: 1.3e-3 at 2.5, 3.7e-3 at 3.5, 4.5e-3 at 5, where the emulation (2.9e-4) leaves its bound; input_layernorm.bias x 10
(the padding rows' q and k are that bias alone) gives 5.6e-4.

Recorded and not asserted (TILE_RECORDED_ONLY): tanh-GELU for erf-GELU, 2.7e-5.  Levers tried, at q / k x 2.5: fc1.bias - 3.0
for - 2.5 gives 1.7e-5, fc1.bias - 3.5 with fc2.weight x 30 gives 5.1e-5: the two forms differ by 4.7e-4 absolute at most, which a
residual stream does not carry.  tests/test_gpu_gemm.py::test_gelu_dense_grid_fast_and_slow_path (mutant "tanh-GELU") holds the
erf-GELU epilogue the tile tower runs apart from the other form element by element.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import tile_reference as tr  # noqa: E402
import tower_mutants as tm  # noqa: E402

GEOM = tm.TILE_GEOM
TWO_TILES = 1  # the index of the 2-tile image
_cache = {}


def weights(sharp: bool = True) -> dict:
    if ("w", sharp) not in _cache:
        _cache["w", sharp] = tm.tile_weights(sharp)
    return _cache["w", sharp]


def inputs() -> list:
    if "x" not in _cache:
        _cache["x"] = tm.tile_inputs()
    return _cache["x"]


def restatement(k: int, sharp: bool = True):
    """(the state behind the stem and the local layer, the outputs) of the float32 restatement on image k, computed once"""
    if ("f32", k, sharp) not in _cache:
        local = tr.local_state(*inputs()[k], weights(sharp), GEOM, torch.float32)
        _cache["f32", k, sharp] = (local, tr.tile_outputs(*inputs()[k], weights(sharp), GEOM, torch.float32, None, local))
    return _cache["f32", k, sharp]


def mutant_distance(name: str, k: int = TWO_TILES, sharp: bool = True) -> dict:
    """output -> max(1 - cos) of the float32 mutant `name` from the float32 restatement on image k; the mutants that leave the stem
    and the local layer alone start from the restatement's state behind them"""
    local, want = restatement(k, sharp)
    got = tr.tile_outputs(*inputs()[k], weights(sharp), GEOM, torch.float32, name, local if name in tr.LOCAL_FREE else None)
    return {out: float(tm.one_minus_cos(got[out], want[out]).max()) for out in want}


def test_tile_reference_is_the_oracle_bit_for_bit():
    from oracle import mllama_vision as om

    pv, aid, nt = inputs()[TWO_TILES]
    want = om.vision_forward(pv, aid, nt, weights(), GEOM)
    got = tr.vision_forward(pv, aid, nt, weights(), GEOM, torch.float32)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)
    out = restatement(TWO_TILES)[1]  # ... and from the saved local state; the pooled vector is the oracle's
    assert np.array_equal(out["final"], want[:, :, : GEOM.hidden_size]) and np.array_equal(out["intermediate 0"], want[:, :, GEOM.hidden_size :])
    assert np.abs(out["pooled"][0, 0] - om.pooled_embedding(want)).max() <= 1e-7


@pytest.mark.parametrize("k", range(len(tm.TILE_IMAGES)), ids=["1 tile", "2 tiles", "4 tiles"])
def test_float32_and_the_bf16_emulation_stay_near_float64(k):
    pv, aid, nt = inputs()[k]
    assert nt == (1, 2, 4)[k] and aid == (1, 2, 6)[k] and not pv[nt:].any()
    f64 = tr.tile_outputs(pv, aid, nt, weights(), GEOM, torch.float64)
    f32 = tm.tile_distance(restatement(k)[1], f64)
    bf16 = tm.tile_distance(tr.tile_outputs(pv, aid, nt, weights(), GEOM, torch.float32, "bf16"), f64)
    print(f"\n{nt} tile(s): float32 {f32:.2e}, bf16 emulation {bf16:.2e} from float64")
    assert f32 <= tm.EMULATION_NEAR / 10, (nt, f32)
    assert bf16 <= tm.EMULATION_NEAR, (nt, bf16)


@pytest.mark.parametrize("label", list(tm.TILE_MUTANTS))
def test_sharp_weights_separate_every_required_mutant(label):
    d = mutant_distance(tm.TILE_MUTANTS[label])
    print(f"\n{label}: " + ", ".join(f"{out} {v:.2e}" for out, v in d.items()))
    assert max(d.values()) >= tm.MUTANT_FAR, (label, d)


@pytest.mark.parametrize("label", list(tm.TILE_RECORDED_ONLY))
def test_recorded_only_mutants_are_measured(label):
    """Recorded, not asserted (the docstring above says why, and which kernel-level test holds the property)"""
    d = mutant_distance(tm.TILE_RECORDED_ONLY[label])
    print(f"\n{label} (recorded only): " + ", ".join(f"{out} {v:.2e}" for out, v in d.items()))
    assert all(np.isfinite(v) for v in d.values())


def test_the_required_tile_mutants_are_registered():
    need = {"uniform attention", "Q and K exchanged", "no dh^-0.5", "heads rolled by one between P and V",
            "padding keys masked for every query", "(padding, padding) mask dropped", "each tile attends only itself",
            "global gates ignored", "gate used without its tanh", "gate_attn / gate_ffn exchanged",
            "pre-tile embedding added to the class row too", "(1 - tanh g) factor dropped", "tile-embedding rows rolled by one tile",
            "post-tile embedding left out", "post-tile embedding added before layernorm_post", "layernorm_pre left out",
            "layernorm_post left out", "ln1 / ln2 parameters exchanged", "residual around the MLP dropped",
            "the class row of tile 1 pooled for tile 0"}
    assert need <= set(tm.TILE_MUTANTS), need - set(tm.TILE_MUTANTS)
    assert set(tm.TILE_RECORDED_ONLY) <= {"a tile's 7 padding tokens taken as real", "one key of 6432 dropped", "tanh-GELU for erf-GELU"}
    assert not set(tm.TILE_RECORDED_ONLY) & set(tm.TILE_MUTANTS)
    assert (GEOM.num_layers, GEOM.num_global_layers, GEOM.intermediate_layers) == (1, 1, (0,))
    w = weights()
    gates = {name: float(v[0]) for name, v in w.items() if name.endswith("gate") or ".gate_" in name}
    assert len(gates) == 5 and all(gates.values()), gates
    assert gates["global_transformer.layers.0.gate_attn"] != gates["global_transformer.layers.0.gate_ffn"]
    assert all(np.array_equal(v, tm.W.round_to_bf16(v).reshape(v.shape)) for v in w.values()), "every value is a bf16 value"


if __name__ == "__main__":  # the table of the docstring: the sharp weights beside the unmodified make_tile_vit_weights
    t0 = time.time()
    rows = []
    for label, name in {**tm.TILE_MUTANTS, **tm.TILE_RECORDED_ONLY}.items():
        rows.append((label, max(mutant_distance(name).values()), max(mutant_distance(name, sharp=False).values())))
    pv, aid, nt = inputs()[TWO_TILES]
    for sharp in (True, False):
        f64 = tr.tile_outputs(pv, aid, nt, weights(sharp), GEOM, torch.float64)
        rows.insert(0 if sharp else 1, ("bf16 emulation, from float64" if sharp else "", tm.tile_distance(
            tr.tile_outputs(pv, aid, nt, weights(sharp), GEOM, torch.float32, "bf16"), f64), None))
    emu = rows.pop(1)[1]
    rows[0] = (rows[0][0], rows[0][1], emu)
    print(f"    {'the 2-tile image, max(1 - cos) over all outputs':56s} {'sharp weights':>14s} {'make_tile_vit_weights':>22s}")
    for label, a, b in rows:
        print(f"    {label:56s} {a:14.1e} {b:22.1e}")
    unseen = [label for label, _, b in rows[1:] if label in tm.TILE_MUTANTS and b < tm.BOUND]
    print(f"    inside the 1e-3 bound at make_tile_vit_weights: {', '.join(unseen)}")
    print(f"    ({time.time() - t0:.0f} s)")
