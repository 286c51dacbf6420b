"""The tile tower on the GPU against its restatement, on the sharp weights of tests/tower_mutants.py (the tile case).

tests/test_gpu_tilevit.py holds max(1 - cos) <= 1e-3 per token on `make_tile_vit_weights`, where the 6432-key softmax is nearly
flat and both gates of a global layer are pi / 4: tests/test_tile_tower_sharpness_cpu.py lists the wrong towers which that bound
cannot see there (uniform attention, the (padding, padding) mask dropped, the global gates ignored or exchanged, ...) and shows
that on the sharp weights every required one is at least 4e-3 from the restatement, while the restatement's bf16 emulation
stays within 2.5e-4 of float64 and its float32 form within 2.5e-5.  Here the engine runs those weights (`load_tile_vit`) on the
same three images of 1, 2 and 4 tiles (`mme_preprocess_tiles`, checked to give the pixel values the CPU test uses), through
`tile_vit_forward(want_hidden=True)` under set_ln_fusion 2 and 1 x set_attention_mode 1 (the fast form with its guard) and 0
(the exact form).

Asserted, per setting: every row of all four tiles (the padding tiles included: they are where the mask shows) of the final-state
slice and of the intermediate slice (the engine's row de-interleaved by its `d * k + layer` layout; kept apart so that a wide
row does not dilute a wrong slice), and the pooled vector, are within 1e-3 (the project's bound) of the float32 restatement,
which is computed once per image.  By the triangle inequality on angles an engine that passes is more than 1e-3 from every
required mutant.  Also: the two ln_fusion modes give the same bits, emb_bf16 is the rounded emb_f32, the pooled vector has unit
norm.  Printed, not asserted: the worst distance per output, and the `attention_redone` words of the fast form (sharp scores
may legitimately trip the guard).

Observed on an MI355X (`pytest -s` prints them), max(1 - cos) over the rows of all four tiles, fast / exact attention form (the
two ln_fusion modes give the same bits, so the same figures):

                           final state          intermediate (local layer)               pooled
    1 tile     8.99e-05 / 8.27e-05         6.28e-05 / 6.23e-05         2.69e-05 / 2.12e-05
    2 tiles    1.42e-04 / 1.34e-04         6.43e-05 / 6.39e-05         2.65e-05 / 2.75e-05
    4 tiles    1.44e-04 / 1.42e-04         8.71e-05 / 8.52e-05         2.56e-05 / 2.81e-05

`attention_redone` of the fast form: [0, 0] (local, global) under both ln_fusion modes: at q / k x 4 the fast form stands.  Beside
it, from the CPU test on the same weights and images: the bf16 emulation of the restatement is 8.5e-5, 1.3e-4 and 9.3e-5 from
float64, so the engine sits where an honest bf16 path is expected; the nearest required mutant is 4.1e-3 away.  Check of the checks:
with "gate_attn / gate_ffn exchanged" in place of the restatement all four settings fail, on every image, at 3.3e-2 to 3.5e-2 on the
final-state slice and 1.4e-2 to 1.5e-2 on the pooled vector.  The module takes 20 s, 17 of them the three restatement passes.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tile_reference as tr  # noqa: E402
import tower_mutants as tm  # noqa: E402

from multimodal_embeddings_amd._lib import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = [(2, 1), (2, 0), (1, 1), (1, 0)]  # (set_ln_fusion, set_attention_mode)
N_LAYERS = tm.TILE_GEOM.num_layers + tm.TILE_GEOM.num_global_layers
_fault = []
_state = {}


@pytest.fixture(autouse=True)
def _a_fault_ends_the_module():
    if _fault:
        pytest.fail(f"not run: an earlier test of this module met a GPU fault ({_fault[0]})")
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _fault.append(str(e)[:200])
        raise


def reference(pv, ids, nt, w) -> list:
    """Per image the outputs of the float32 restatement; the check of the checks puts a required mutant here"""
    return [tr.tile_outputs(pv[k], int(ids[k]), int(nt[k]), w, tm.TILE_GEOM, torch.float32) for k in range(len(nt))]


def runs() -> dict:
    """Everything the tests below look at, computed once: the engine's outputs under the four settings (host arrays), the redo
    words of each run, and the restatement's outputs per image"""
    if _state:
        return _state
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    w = tm.tile_weights()
    eng = Engine(0)
    try:
        eng.load_tile_vit(w, tm.TILE_GEOM)
        pix, offs, hw = RegionEmbedder(engine=eng).pack(tm.tile_images())
        pv, ids, _, nt = eng.preprocess_tiles(pix, offs, hw, 560, 4)
        torch.cuda.synchronize()
        got = {}
        for ln, mode in SETTINGS:
            eng.set_ln_fusion(ln)
            eng.set_attention_mode(mode)
            hidden, e32, e16 = eng.tile_vit_forward(pv, ids, nt, want_hidden=True)
            torch.cuda.synchronize()
            got[ln, mode] = (hidden.cpu().numpy(), e32.cpu().numpy(), e16.float().cpu().numpy(), e32.to(torch.bfloat16).float().cpu().numpy(),
                             eng.attention_redone(N_LAYERS + 2))
        pvh = pv.cpu().numpy()
    finally:
        eng.close()
    inputs = tm.tile_inputs()
    assert [int(n) for n in nt] == [n for _, _, n in inputs] == [1, 2, 4]
    assert [int(i) for i in ids] == [a for _, a, _ in inputs] and len(set(int(i) for i in ids)) == 3
    assert all(np.array_equal(pvh[k], inputs[k][0]) for k in range(3)), "the pixel values of the CPU test"
    _state.update(got=got, want=reference(pvh, ids, nt, w), nt=[int(n) for n in nt])
    return _state


def engine_outputs(hidden, e32, k: int) -> dict:
    """Image k of a run under the names of tile_reference.tile_outputs"""
    return {**tr.split_row(hidden[k], tm.TILE_GEOM), "pooled": np.asarray(e32[k], dtype=np.float64)[None, None, :]}


@pytest.mark.parametrize("ln_fusion,attention_mode", SETTINGS, ids=[f"ln_fusion_{a}-attention_{'fast' if m else 'exact'}" for a, m in SETTINGS])
def test_sharp_tile_tower_is_within_the_bound_of_the_restatement(ln_fusion, attention_mode):
    s = runs()
    hidden, e32, _, _, redone = s["got"][ln_fusion, attention_mode]
    assert hidden.shape == (3, 4, 1601, tm.TILE_GEOM.output_dim) and np.isfinite(hidden).all() and np.isfinite(e32).all()
    assert redone[N_LAYERS:] == [0, 0], redone
    if attention_mode:
        print(f"ln_fusion {ln_fusion}, fast attention: attention_redone per layer (local, global) of the last pass {redone[:N_LAYERS]}")
    failed = []
    for k, want in enumerate(s["want"]):
        got = engine_outputs(hidden, e32, k)
        assert got.keys() == want.keys() and all(got[name].shape == want[name].shape for name in want)
        worst = {name: tm.one_minus_cos(got[name], want[name]) for name in want}
        print(f"ln_fusion {ln_fusion}, attention {'fast' if attention_mode else 'exact'}, {s['nt'][k]} tile(s): max(1 - cos) "
              + ", ".join(f"{name} {err.max():.3g}" for name, err in worst.items()))
        failed += [(s["nt"][k], name, float(err.max()), np.unravel_index(err.argmax(), err.shape)) for name, err in worst.items()
                   if not err.max() <= tm.BOUND]
    assert not failed, failed


def test_settings_identities_and_the_pooled_vector():
    """What tests/test_gpu_tilevit.py asserts of the shallow tower, on the sharp weights: the two ln_fusion modes give the same
    bits under either attention form, emb_bf16 is emb_f32 rounded, the pooled vector has unit norm"""
    got = runs()["got"]
    for mode in (1, 0):
        a, b = got[2, mode], got[1, mode]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), mode
    for key, (_, e32, e16, e32_rounded, _) in got.items():
        assert np.array_equal(e16, e32_rounded), key
        assert np.abs(np.linalg.norm(e32.astype(np.float64), axis=1) - 1.0).max() <= 1e-5, key
