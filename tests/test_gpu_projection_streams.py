"""mme_moments and mme_project run on the caller's stream: probes A and B of tests/stream_probes.py (its docstring says what each
sees), the standard tests/test_gpu_streams.py holds every other asynchronous entry point to.  A fresh Engine per probe, so the
first-call path (`ensure` of the workspace) runs under it.  Sharpness: the same calls made with stream = NULL while the side
stream is current must be noticed by both probes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import projection_reference as PJ  # noqa: E402
import stream_probes as sp  # noqa: E402
from stream_probes import DEV, Case  # noqa: E402

from multimodal_embeddings_amd._lib import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, M = 2 * PJ.BLOCK + 3, 128, 64  # three row blocks, an off-diagonal tile; 33 row tiles of the projection
RECORD = {}


def setup():
    return Engine(0)


@functools.lru_cache(maxsize=None)
def inputs(v):
    """v = 0, 1: two real tables with their mean and weights; v = 2: the poison, as valid as they are"""
    rng = np.random.default_rng(1700 + v)
    x = rng.standard_normal((N, D)) + 0.5 * (v + 1)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    bits = torch.from_numpy(PJ.to_bf16_bits(x).view(np.int16)).view(torch.bfloat16)
    w = np.linalg.qr(rng.standard_normal((D, M)))[0].T * np.logspace(0, 1, M)[:, None]
    return {"emb": bits, "mean": torch.from_numpy(x.mean(axis=0).astype(np.float32)), "w": torch.from_numpy(w.astype(np.float32))}, {}


def _raw(eng, name, *args):
    rc = getattr(eng.lib, name)(eng.h, *args)
    assert rc == 0, eng.lib.mme_last_error(eng.h).decode()


def call_moments(eng, d, h, null=False):
    if not null:
        s, g = eng.moments(d["emb"])
        return {"sum": s, "gram": g}
    s = torch.full((D,), 3.0, dtype=torch.float64, device=DEV)
    g = torch.full((D, D), 3.0, dtype=torch.float64, device=DEV)
    _raw(eng, "mme_moments", d["emb"].data_ptr(), N, D, s.data_ptr(), g.data_ptr(), None)
    return {"sum": s, "gram": g}


def call_project(eng, d, h, null=False):
    """both outputs of one call: the row kernel reads the caller's f32 rows"""
    if not null:
        y16, y32 = eng.project(d["emb"], d["mean"], d["w"], f32=True)
        return {"y16": y16, "y32": y32}
    y32 = torch.full((N, M), 3.0, dtype=torch.float32, device=DEV)
    y16 = torch.full((N, M), 3.0, dtype=torch.bfloat16, device=DEV)
    _raw(eng, "mme_project", d["emb"].data_ptr(), N, D, d["mean"].data_ptr(), d["w"].data_ptr(), M, y32.data_ptr(), M, y16.data_ptr(), None)
    return {"y16": y16, "y32": y32}


def call_project_rows_only(eng, d, h, null=False):
    """the normalised rows alone: the f32 rows go through the workspace, which two calls in flight share"""
    if not null:
        return {"y16": eng.project(d["emb"], d["mean"], d["w"])}
    y16 = torch.full((N, M), 3.0, dtype=torch.bfloat16, device=DEV)
    _raw(eng, "mme_project", d["emb"].data_ptr(), N, D, d["mean"].data_ptr(), d["w"].data_ptr(), M, None, 0, y16.data_ptr(), None)
    return {"y16": y16}


CALLS = {"moments": ("moments", call_moments), "project": ("project", call_project), "project-rows-only": ("project", call_project_rows_only)}
CASES = {label: Case(entry, label, setup, inputs, call) for label, (entry, call) in CALLS.items()}


def _record(entry, probe, effective, label):
    RECORD.setdefault((entry, probe), []).append(bool(effective))
    print(f"{label:20s} probe {probe}: the delay was {'still pending' if effective else 'over'} when it mattered")


@pytest.mark.parametrize("label", list(CASES))
def test_probe_a_busy_null_stream(label):
    bad, effective = sp.probe_a(CASES[label])
    _record(CASES[label].entry, "A", effective, label)
    assert not bad, (label, bad)


@pytest.mark.parametrize("label", list(CASES))
def test_probe_b_late_input_back_to_back(label):
    bad, effective = sp.probe_b(CASES[label])
    _record(CASES[label].entry, "B", effective, label)
    assert not bad, (label, bad)


@pytest.mark.parametrize("probe", ["A", "B"])
@pytest.mark.parametrize("label", list(CASES))
def test_a_call_on_the_null_stream_is_seen(label, probe):
    bad, effective = (sp.probe_a if probe == "A" else sp.probe_b)(CASES[label], functools.partial(CALLS[label][1], null=True))
    print(f"{label} with stream = NULL, probe {probe}: differs in {bad}, effective {effective}")
    assert effective, "the delay ran out before the probe looked: the harness is too weak to see a wrong stream"
    assert bad, "a call enqueued on the null stream went unnoticed"


def test_both_entry_points_have_an_effective_probe():  # keep last
    entries = sorted({c.entry for c in CASES.values()})
    if not all((e, p) in RECORD for e in entries for p in "AB"):
        pytest.fail("the probes above did not all run: the table is incomplete")
    weak = [e for e in entries if not any(any(v) for (n, _), v in RECORD.items() if n == e)]
    assert not weak, f"no effective probe: {weak}"
