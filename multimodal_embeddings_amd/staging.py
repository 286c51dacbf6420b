"""What the two host pipelines share: `RegionEmbedder._embed_list` and `RegionProcessor.process_regions`.

Both feed the device from a producer thread while the calling thread runs the passes and the rows of the pass before go back
to the host.  Written once here: the packed-crop layout, the stream / event stand-ins that let either pipeline run on CPU
tensors with a stand-in engine, the producer / consumer skeleton (`Stage`) and the one-behind pinned result buffers
(`ResultRing`).  What a producer stages and what a consumer does with a message stay with the pipelines.

The rule neither class can enforce: every `Engine` call belongs to the consumer -- the thread that opened the `Stage`.  A
producer decodes, copies host memory and enqueues H2D copies on its own stream, nothing else.
"""
from __future__ import annotations

import contextlib
import queue
import threading

import numpy as np


# -- packed crops ------------------------------------------------------------------------------------------------------
def aligned(nbytes):
    """Bytes (an int or an int64 array) rounded up to the 16-byte alignment every packed crop starts on."""
    return (nbytes + 15) // 16 * 16


def packed_layout(hw):
    """(h, w) int32[n, 2] of uint8 RGB crops -> (offs int64[n], sizes int64[n], total): each crop starts on 16 bytes behind
    the one before it, and `total` leaves 16 bytes behind the last (K1 reads whole 16-byte words); 16 for no crops."""
    hw = np.asarray(hw).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(len(sizes), dtype=np.int64)
    if len(sizes) > 1:
        offs[1:] = np.cumsum(aligned(sizes[:-1]))
    total = int(offs[-1] + sizes[-1]) + 16 if len(sizes) else 16
    return offs, sizes, total


def packed_bytes(hw) -> int:
    """What the crops `hw` take of a packed buffer that goes on behind them: the 16-byte aligned start of the next crop."""
    hw = np.asarray(hw).reshape(-1, 2)
    return int(aligned(hw[:, 0].astype(np.int64) * hw[:, 1] * 3).sum())


# -- streams and events, or nothing ---------------------------------------------------------------------------------------
class _Null:
    """Stream / event stand-in where there is no device (host-logic tests): every ordering call is a no-op."""

    def wait_event(self, *_):
        pass

    def record(self, *_):
        pass

    def synchronize(self):
        pass


def new_stream(dev):
    import torch

    return torch.cuda.Stream(dev) if dev.type == "cuda" else _Null()


def new_event(dev):
    import torch

    return torch.cuda.Event() if dev.type == "cuda" else _Null()


def current_stream(dev):
    """The calling thread's compute stream on `dev`."""
    import torch

    return torch.cuda.current_stream(dev) if dev.type == "cuda" else _Null()


def on(dev, stream=None):
    """Context manager: `dev` current (and `stream` current on it); nothing to do without a device."""
    import torch

    if dev.type != "cuda":
        return contextlib.nullcontext()
    return torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev)


# -- producer thread / consuming caller -------------------------------------------------------------------------------------
class Stage:
    """`produce(stage)` on a thread of its own feeding the thread that opened the stage, over a queue bounded by `slots`:

        with Stage(name, produce, slots, dev, log) as stage:
            for msg in iter(stage.get, None): ...

    The producer takes a slot (`acquire`) before it fills the buffers behind it and hands it over in a message (`put`); the
    consumer gives it back (`release`) once the device work that reads those buffers is enqueued and an event recorded
    behind it.  `get` returns None once the producer has returned or raised (logged, as a failed batch): the consumer is
    never left waiting.  Leaving the block -- through an exception too, after a device synchronize, so that nothing stays in
    flight on buffers the next call reuses -- stops the producer wherever it waits and joins it."""

    def __init__(self, name, produce, slots, dev, log):
        self.dev, self.log = dev, log
        self.ready = queue.Queue(maxsize=slots)
        self.free = [threading.Semaphore(1) for _ in range(slots)]
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._run, args=(produce,), name=name, daemon=True)

    def _run(self, produce):
        try:
            produce(self)
        except BaseException as e:  # never leave the consumer waiting
            self.log.error(f"Error in batch processing: {e}")
        finally:
            self.ready.put(None)

    def acquire(self, slot) -> bool:
        """Producer: wait for `slot`; False when the consumer has left and the producer should return."""
        while not self.free[slot].acquire(timeout=0.1):
            if self.stop.is_set():
                return False
        return True

    def release(self, slot):
        self.free[slot].release()

    def put(self, msg):
        self.ready.put(msg)

    def get(self):
        return self.ready.get()

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is not None and self.dev.type == "cuda":
                import torch

                torch.cuda.synchronize(self.dev)
        finally:
            self.stop.set()
            while self.thread.is_alive():  # drain so that a blocked put() returns
                try:
                    self.ready.get(timeout=0.05)
                except queue.Empty:
                    pass
            self.thread.join()
        return False


# -- rows back to the host, one submission behind ------------------------------------------------------------------------------
class ResultRing:
    """Two pinned float32 [rows, D] buffers (at least `min_rows` rows, regrown when too small or when D changes), a copy
    stream and an event per buffer, kept across calls.  Per call: `start(finalize)`, a `submit` per device pass, `finish()`.

    `submit` enqueues the D2H of a pass's rows on the copy stream and only then hands the submission BEFORE it to
    `finalize(tag, rows)` -- `rows` the numpy view of its buffer, valid until the next `submit` -- so the host work on one
    pass runs under the device work of the next; `finish` hands over the last.  A buffer's pending occupant is always
    finalized before the buffer is written again."""

    def __init__(self, dev, min_rows):
        self.dev, self.min_rows = dev, min_rows
        self.stream = new_stream(dev)
        self.out, self.ev_out = [None, None], [new_event(dev), new_event(dev)]
        self.start(None)

    def start(self, finalize):
        self.finalize, self.pending, self.count = finalize, None, 0  # an earlier call may have left through an exception

    def submit(self, rows, after, tag):
        """rows: f32 device tensor [n, D] of a pass; after: an event recorded on the compute stream behind that pass."""
        import torch

        b = self.count & 1
        self.count += 1
        n, d = rows.shape
        if self.pending is not None and self.pending[0] == b:
            self._finalize_pending()  # this buffer is about to be reused
        if self.out[b] is None or self.out[b].shape[0] < n or self.out[b].shape[1] != d:
            self.out[b] = torch.empty((max(n, self.min_rows), d), dtype=torch.float32, pin_memory=self.dev.type == "cuda")
        with on(self.dev, self.stream):
            self.stream.wait_event(after)
            self.out[b][:n].copy_(rows, non_blocking=True)
            self.ev_out[b].record(self.stream)
        if self.pending is not None:
            self._finalize_pending()  # the host's share of the previous pass, under this one's device work
        self.pending = (b, n, tag, rows)  # `rows` kept alive while its copy is in flight

    def finish(self):
        if self.pending is not None:
            self._finalize_pending()

    def _finalize_pending(self):
        b, n, tag, _keep = self.pending
        self.pending = None
        self.ev_out[b].synchronize()
        self.finalize(tag, self.out[b][:n].numpy())
