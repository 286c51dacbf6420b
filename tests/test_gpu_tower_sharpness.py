"""Whole towers on the GPU against the float64 restatements, on the sharp weights of tests/tower_mutants.py.

The end-to-end tests elsewhere hold max(1 - cos) <= 1e-3 on `make_*_weights(std=0.02)`, where the softmax is nearly flat:
tests/test_tower_sharpness_cpu.py lists the wrong towers that bound cannot see there (uniform attention, Q and K exchanged, a
dropped key, the other activation) and shows that on the sharp weights every one of them is at least 4e-3 from the
restatement, while the restatement's own bf16 emulation stays below 2.5e-4.  Here the engine runs those weights and inputs:

  image towers  Engine.vit_tokens over all token rows, with the pooled output under pool token 0 and under the last token
                (image_embeds for CLIP, whose cases carry the 512-wide projection; the head's output for SigLIP, the same under
                both pool tokens);
  text towers   Engine.text_forward on eight sequences of different lengths;

each at the default settings and with set_ln_fusion(0).  Asserted: max(1 - cos) <= 1e-3 (the project's bound) against the
float64 restatement on every row of every output.  By the triangle inequality on angles an engine that passes is more than
1e-3 from every mutant of the CPU test; the mutants themselves are not run here.  Identities between settings are tested in
the towers' own files and not repeated.

Observed on an MI355X (`pytest -s` prints them), max(1 - cos) over all rows and outputs, default settings / set_ln_fusion(0):

                            token rows       pooled, token 0    pooled, last token          text_forward
    vit_b16        7.98e-05 / 9.48e-05   7.17e-05 / 8.04e-05    5.4e-05 / 4.66e-05                     -
    vit_b32        6.86e-05 / 6.36e-05    6.76e-05 / 6.3e-05   2.36e-05 / 2.52e-05                     -
    vit_s16        6.78e-05 / 6.89e-05   6.61e-05 / 6.31e-05   1.89e-05 / 3.74e-05                     -
    dinov2_b14     2.67e-05 / 2.47e-05   2.37e-05 / 2.26e-05   1.58e-05 / 1.59e-05                     -
    dinov2_1024    8.04e-05 / 8.97e-05    6.68e-05 / 8.3e-05   5.07e-05 / 6.47e-05                     -
    clip_b16       5.49e-05 / 4.83e-05   3.12e-05 / 3.11e-05   3.48e-05 / 3.06e-05                     -
    clip_b32       5.64e-05 / 5.67e-05    3.5e-05 / 3.43e-05    3.79e-05 / 3.5e-05                     -
    siglip_b16     5.72e-05 / 5.97e-05   2.07e-05 / 1.59e-05   2.07e-05 / 1.59e-05                     -
    clip_text                        -                     -                     -     1.1e-05 / 1.1e-05
    siglip_text                      -                     -                     -   2.86e-05 / 2.86e-05

(the text towers do not consult the setting, csrc/capi_text.hip: their second run is the first again.)  Beside it, from the
CPU table of tests/test_tower_sharpness_cpu.py on the same weights and inputs: the bf16 emulation of the restatement is 8e-6
to 8e-5 from float64, so the engine sits where an honest bf16 path is expected; the nearest required mutant of any tower is
6e-3 away ("final LayerNorm left out", ViT-B/32), the formerly invisible ones 1e-2 to 7e-1.  Check of the checks: with "last key
dropped" in place of the restatement the ViT 384, DINOv2-B, CLIP-B/16 and SigLIP-B cases fail at 1.5e-2 to 8.5e-2 on the token
rows.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tower_mutants as tm  # noqa: E402
from test_gpu_gemm import DEV  # noqa: E402

from multimodal_embeddings_amd._lib import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

_fault = []
_cases = {}


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


def case(key):
    """(weights, inputs, float64 outputs of the restatement), computed once per tower and left unchanged"""
    if key not in _cases:
        w, x = tm.weights_of(key), tm.inputs_of(key)
        _cases[key] = (w, x, tm.outputs(key, w, x if tm.TOWERS[key].text else x[1]))
    return _cases[key]


def engine_outputs(eng, key, x) -> dict:
    """The engine's outputs under the names of tm.outputs; an image tower's token rows are checked to be the same bits under
    both pool tokens and returned once"""
    t, geom = tm.TOWERS[key], tm.geom_of(key)
    f64 = lambda v: v.double().cpu().numpy()  # noqa: E731
    if t.text:
        e32, _ = eng.text_forward(x)
        torch.cuda.synchronize()
        return {"text": f64(e32)[:, None, :]}
    crops = x[0]
    n, per = crops.shape[0], int(np.prod(crops.shape[1:]))
    pix = torch.cat([torch.from_numpy(np.ascontiguousarray(crops)).to(DEV).reshape(-1), torch.zeros(16, dtype=torch.uint8, device=DEV)])
    patches = eng.preprocess(pix, np.arange(n, dtype=np.int64) * per, np.full((n, 2), 224, dtype=np.int32))
    T = geom.seq_len
    out, rows = {}, []
    for name, tok in (("pooled 0", 0), ("pooled last", T - 1)):
        tokens, e32, _ = eng.vit_tokens(patches, pool_token=tok, tok0=0, ntok=T)
        torch.cuda.synchronize()
        assert tuple(tokens.shape) == (n, T, geom.hidden_size) and tuple(e32.shape) == (n, eng.embed_dim)
        rows.append(tokens)
        out[name] = f64(e32)[:, None, :]
    assert torch.equal(rows[0].view(torch.int16), rows[1].view(torch.int16)), "the token rows do not depend on the pool token"
    out["tokens"] = f64(rows[0])
    return out


@pytest.mark.parametrize("ln_fusion", [None, 0], ids=["default", "ln_fusion_0"])
@pytest.mark.parametrize("key", list(tm.TOWERS))
def test_sharp_tower_is_within_the_bound_of_the_float64_restatement(key, ln_fusion):
    w, x, want = case(key)
    eng = Engine(0)
    try:
        getattr(eng, tm.LOADER[tm.TOWERS[key].kind])(w, geom=tm.geom_of(key))
        if ln_fusion is not None:
            eng.set_ln_fusion(ln_fusion)
        got = engine_outputs(eng, key, x)
    finally:
        eng.close()
    if tm.TOWERS[key].kind == "siglip":  # the head reads every row: one output, whatever the pool token
        want = {"tokens": want["tokens"], "pooled 0": want["head"], "pooled last": want["head"]}
    assert got.keys() == want.keys()
    worst = {name: tm.one_minus_cos(got[name], want[name]) for name in want}
    print(f"{key} ({'default' if ln_fusion is None else 'set_ln_fusion(0)'}): max(1 - cos) "
          + ", ".join(f"{name} {err.max():.3g}" for name, err in worst.items()))
    for name, err in worst.items():
        assert got[name].shape == want[name].shape and np.isfinite(got[name]).all(), name
        assert err.max() <= tm.BOUND, (key, name, float(err.max()), np.unravel_index(err.argmax(), err.shape))
