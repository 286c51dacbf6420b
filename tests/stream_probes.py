"""Test infrastructure of tests/test_gpu_streams.py: a calibrated delay, the three probes and the reference run.

include/mme.h promises that every launch of an entry point is asynchronous on the caller's `stream`.  A call on an otherwise
idle default stream with a device synchronise behind it cannot tell a library that keeps the promise from one that does not.
The probes here can:

  Delay     a chain of in-place elementwise torch operations on one 512 MiB tensor, calibrated once with events to
            TARGET_MS (never below MIN_MS, never above MAX_MS).  No spin kernel, no graph capture, no environment.
  probe_a   the delay sits on the DEFAULT stream; the call is made on an idle side stream and its outputs are copied on that
            stream at once; the side stream is synchronised and the copies are what is compared.  A step the result depends
            on that went to the null stream lands behind the delay and arrives too late.
  probe_b   the side stream itself carries the delay, then the device-to-device copies of the real inputs over a poison (another
            valid input), then the call; the same again with a second input and no host synchronisation; after each call returns
            the caller's host arrays are overwritten in place with other valid contents.  Both results must be those of the
            contents at call time: a step on another stream reads the poison, scratch shared by the two calls in flight mixes
            them, a host array read late gives the overwrite.
  reference the same call on a fresh engine on the default stream between two device synchronises; compared bit for bit
            (`Case.canon` puts outputs whose order is arbitrary into a canonical one first).

A probe returns (names of the outputs that differ, effective): `effective` says that an event recorded behind the delay was
still pending when it mattered, i.e. that the probe could have seen a violation.  A delay that ran out makes a probe weaker,
never red.  Every output buffer is scribbled over once it has been read back, so that a later run cannot find the right
answer lying in a block the allocator hands out again.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

DEV = torch.device("cuda", 0)


class Delay:
    TARGET_MS, MIN_MS, MAX_MS = 140.0, 40.0, 200.0

    def __init__(self, numel: int = 1 << 27):
        self.buf = torch.ones(numel, dtype=torch.float32, device=DEV)
        self.iters, self.ms = self._calibrate()

    def _chain(self, n):
        for _ in range(n):
            self.buf.neg_()  # in place, bounded for ever

    def _time(self, n) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        self._chain(n)
        b.record()
        b.synchronize()
        return float(a.elapsed_time(b))

    def _calibrate(self):
        self._time(64)  # clocks up
        n = max(1, math.ceil(self.TARGET_MS / (self._time(64) / 64)))
        ms = self._time(n)
        for _ in range(4):
            if self.TARGET_MS * 0.85 <= ms <= self.TARGET_MS * 1.15:
                break
            n = max(1, math.ceil(n * self.TARGET_MS / ms))
            ms = self._time(n)
        assert self.MIN_MS <= ms <= self.MAX_MS, (n, ms)
        return n, ms

    def enqueue(self, stream, part: int = 1):
        """The chain (1 / part of it) on `stream` -> an event recorded behind it"""
        with torch.cuda.stream(stream):
            self._chain(max(1, self.iters // part))
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev


_delay = []


def delay() -> Delay:
    if not _delay:
        _delay.append(Delay())
    return _delay[0]


_streams, _shared = [], []


def side_streams(n: int = 1) -> list:
    """n of (up to) three streams, made once, whose work does not queue behind the null stream's.  The runtime maps streams onto
    a few hardware queues; a stream that shares the null stream's queue runs in its order whatever the library does, and a probe
    on it sees nothing.  Each candidate is tried: a quarter of the delay on the null stream, one small kernel on the candidate,
    which must be done while the delay is still pending."""
    if not _streams:
        d, word = delay(), torch.zeros(64, device=DEV)
        while len(_streams) < 3 and len(_streams) + len(_shared) < 8:
            s = torch.cuda.Stream(DEV)
            torch.cuda.synchronize()
            ev = d.enqueue(torch.cuda.default_stream(DEV), part=4)
            with torch.cuda.stream(s):
                word.add_(1.0)
            s.synchronize()
            (_shared if ev.query() else _streams).append(s)  # the others are kept, so that the mapping stays as it was tried
            torch.cuda.synchronize()
        assert _streams, "every stream tried runs in the null stream's order: the probes cannot see anything"
    return [_streams[i % len(_streams)] for i in range(n)]


@dataclass
class Case:
    """One probed call.
    entry    the entry point's name in the effectiveness table;
    label    the test id;
    setup    () -> a fresh, configured Engine (runs on the default stream; the harness synchronises behind it);
    inputs   (v) -> (device inputs: name -> CPU tensor, caller host arrays: name -> numpy array), v = 0, 1 two different real
             inputs, v = 2 the poison: all three valid and of one shape; computed once and left unchanged;
    call     (engine, device inputs on the GPU, host arrays) -> name -> CUDA tensor | numpy array | None, made under the
             current stream; it passes the host arrays on as they are, so that the library reads the caller's memory;
    canon    name -> host array of all outputs -> the same in a canonical order (where the entry point's order is arbitrary);
    ref_setup  the engine of the reference run when it differs from `setup` (a setting that must not change a bit)."""

    entry: str
    label: str
    setup: Callable
    inputs: Callable
    call: Callable
    canon: Callable | None = None
    ref_setup: Callable | None = None


def to_device(dev_inputs: dict) -> dict:
    return {k: v.to(DEV) for k, v in dev_inputs.items()}


def host_copy(host: dict) -> dict:
    return {k: np.array(v, copy=True) for k, v in host.items()}


def _snapshot(outs: dict) -> dict:
    """copies on the current stream, enqueued at once"""
    return {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in outs.items() if v is not None}


def _bits(outs: dict, canon) -> dict:
    got = {}
    for k, v in outs.items():
        if v is None:
            continue
        if torch.is_tensor(v):
            a = v.contiguous()
            a = a.view(torch.int16) if a.dtype == torch.bfloat16 else a
            got[k] = a.cpu().numpy()
        else:
            got[k] = np.asarray(v)
    return canon(got) if canon else got


def _scribble(*many):
    for outs in many:
        for v in outs.values():
            if torch.is_tensor(v) and v.numel():
                v.fill_(7)


def _differs(got: dict, want: dict) -> list:
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [k for k in want if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]


_refs = {}


def reference(case: Case, v: int) -> dict:
    key = (case.label, v)
    if key not in _refs:
        eng = (case.ref_setup or case.setup)()
        try:
            dev_in, host = case.inputs(v)
            dev_in, host = to_device(dev_in), host_copy(host)
            torch.cuda.synchronize()
            outs = case.call(eng, dev_in, host)
            torch.cuda.synchronize()
            _refs[key] = _bits(outs, case.canon)
            _scribble(outs)
            torch.cuda.synchronize()
        finally:
            eng.close()
    return _refs[key]


def probe_a(case: Case, call=None):
    """-> (outputs that differ from the reference, effective).  `call` replaces case.call (the sharpness cases)"""
    call = call or case.call
    want = reference(case, 0)
    d = delay()
    eng = case.setup()
    try:
        dev_in, host = case.inputs(0)
        dev_in, host = to_device(dev_in), host_copy(host)
        s = side_streams()[0]
        torch.cuda.synchronize()
        ev = d.enqueue(torch.cuda.default_stream(DEV))
        with torch.cuda.stream(s):
            outs = call(eng, dev_in, host)
            copies = _snapshot(outs)
        s.synchronize()
        effective = not ev.query()
        torch.cuda.synchronize()
        bad = _differs(_bits(copies, case.canon), want)
        _scribble(outs, copies)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return bad, effective


def probe_b(case: Case, call=None):
    """-> (outputs that differ from their reference, "call 0: name" / "call 1: name"; effective)"""
    call = call or case.call
    want = [reference(case, 0), reference(case, 1)]
    d = delay()
    eng = case.setup()
    try:
        real = [to_device(case.inputs(v)[0]) for v in (0, 1)]
        poison_dev, poison_host = case.inputs(2)
        dev_in = to_device(poison_dev)
        s = side_streams()[0]
        torch.cuda.synchronize()
        outs, hosts = [], []
        with torch.cuda.stream(s):
            ev = d.enqueue(s)
            for v in (0, 1):
                for k in dev_in:
                    dev_in[k].copy_(real[v][k], non_blocking=True)
                host = host_copy(case.inputs(v)[1])
                outs.append(call(eng, dev_in, host))
                for k in host:  # the call has returned: the arrays are the caller's again
                    np.copyto(host[k], poison_host[k])
                hosts.append(host)
            effective = not ev.query()
        torch.cuda.synchronize()
        bad = [f"call {v}: {k}" for v in (0, 1) for k in _differs(_bits(outs[v], case.canon), want[v])]
        _scribble(*outs)
        torch.cuda.synchronize()
        del hosts, real
    finally:
        eng.close()
    return bad, effective


def chain_c(steps, inputs: dict, canon=None):
    """Probe C.  steps: a list of (engine, (engine, values) -> new values); each step runs on a stream of its own (three in
    turn), which waits on an event recorded behind the step before, while the default stream carries the delay.  `values`
    is a dict that every step adds to.  -> (the bits of every tensor in values behind the last step, effective)"""
    d = delay()
    streams = side_streams(min(3, len(steps)))
    values = dict(inputs)
    torch.cuda.synchronize()
    ev = d.enqueue(torch.cuda.default_stream(DEV))
    done = None
    for i, (eng, step) in enumerate(steps):
        s = streams[i % len(streams)]
        with torch.cuda.stream(s):
            if done is not None:
                s.wait_event(done)
            values.update(step(eng, values))
            done = torch.cuda.Event()
            done.record(s)
    with torch.cuda.stream(s):
        copies = _snapshot({k: v for k, v in values.items() if k not in inputs})
    s.synchronize()
    effective = not ev.query()
    torch.cuda.synchronize()
    got = _bits(copies, canon)
    _scribble({k: v for k, v in values.items() if k not in inputs}, copies)
    torch.cuda.synchronize()
    return got, effective


def chain_reference(steps, inputs: dict, canon=None):
    """The same steps on the default stream, a device synchronise around each"""
    values = dict(inputs)
    for eng, step in steps:
        torch.cuda.synchronize()
        values.update(step(eng, values))
        torch.cuda.synchronize()
    outs = {k: v for k, v in values.items() if k not in inputs}
    got = _bits(outs, canon)
    _scribble(outs)
    torch.cuda.synchronize()
    return got
