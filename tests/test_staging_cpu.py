"""The machinery the two host pipelines share (multimodal_embeddings_amd/staging.py), on CPU tensors with no device: the packed
layout, the producer / consumer skeleton, the one-behind result ring; and the serial embed path on a stand-in engine."""
import logging
import threading

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import embedder as E
from multimodal_embeddings_amd.staging import ResultRing, Stage, packed_bytes, packed_layout

CPU = torch.device("cpu")
LOG = logging.getLogger("test_staging")


def within(fn, seconds=5.0):
    """fn() on a thread of its own under a plain timeout: a regression of the skeleton fails here instead of hanging."""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001 - handed to the test
            box["error"] = e

    th = threading.Thread(target=body, daemon=True)
    th.start()
    th.join(seconds)
    assert not th.is_alive(), f"still running after {seconds} s"
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_packed_layout_is_16_byte_aligned_with_a_16_byte_tail():
    hw = np.array([(1, 1), (2, 3), (16, 16), (5, 7)], dtype=np.int32)
    offs, sizes, total = packed_layout(hw)
    assert sizes.tolist() == [3, 18, 768, 105] and offs.tolist() == [0, 16, 48, 816] and total == 816 + 105 + 16
    assert offs.dtype == np.int64 and sizes.dtype == np.int64
    assert packed_bytes(hw) == 16 + 32 + 768 + 112 and packed_bytes(hw[:3]) == offs[3]
    offs0, sizes0, total0 = packed_layout(np.zeros((0, 2), dtype=np.int32))
    assert len(offs0) == 0 and len(sizes0) == 0 and total0 == 16 and packed_bytes(np.zeros((0, 2), dtype=np.int32)) == 0


def test_pack_lays_crops_out_as_packed_layout():
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(1, 40, (23, 2))]
    emb = E.RegionEmbedder.__new__(E.RegionEmbedder)
    emb.torch, emb.device = torch, CPU
    pix, offs, hw = emb.pack(arrays)
    want_offs, sizes, total = packed_layout(hw)
    assert hw.dtype == np.int32 and hw.tolist() == [list(a.shape[:2]) for a in arrays]
    assert np.array_equal(offs, want_offs) and pix.numel() == total
    for a, o, s in zip(arrays, offs, sizes):
        assert np.array_equal(pix[o : o + s].numpy(), a.reshape(-1))
    assert emb.pack([])[0].numel() == 16


def test_stage_delivers_what_a_failing_producer_sent_then_ends():
    def produce(stage):
        stage.put("a")
        stage.put("b")
        raise RuntimeError("producer broke")

    def call():
        with Stage("stage-test", produce, 2, CPU, LOG) as stage:
            got = list(iter(stage.get, None))
        return got, stage.thread

    got, thread = within(call)
    assert got == ["a", "b"] and not thread.is_alive()


@pytest.mark.parametrize("blocked_in", ["put", "acquire"])
def test_stage_joins_a_blocked_producer_when_the_consumer_raises(blocked_in):
    seen = {}

    def produce(stage):
        if blocked_in == "put":  # far more messages than the queue holds: put() blocks once the consumer has left
            for k in range(50):
                stage.put(k)
            seen["done"] = True
        else:  # the consumer never gives the slot back
            assert stage.acquire(0)
            stage.put("first")
            seen["second acquire"] = stage.acquire(0)

    def call():
        stage = Stage("stage-test", produce, 2, CPU, LOG)
        try:
            with stage:
                for msg in iter(stage.get, None):
                    raise KeyError(msg)
        finally:
            seen["alive"] = stage.thread.is_alive()

    with pytest.raises(KeyError):
        within(call)
    assert seen["alive"] is False
    assert seen.get("done") if blocked_in == "put" else seen["second acquire"] is False


def test_result_ring_finalizes_each_submission_once_in_order_one_behind():
    ring = ResultRing(CPU, 4)
    done = []
    ring.start(lambda tag, rows: done.append((tag, rows.copy())))
    rng = np.random.default_rng(9)
    sent = [torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) for shape in [(3, 3), (6, 3), (2, 3), (5, 4)]]  # 6 > 4 grows, D 3 -> 4
    for k, rows in enumerate(sent):
        ring.submit(rows, None, f"tag{k}")
        assert [tag for tag, _ in done] == [f"tag{j}" for j in range(k)]  # one behind
    ring.finish()
    ring.finish()  # nothing left
    assert [tag for tag, _ in done] == ["tag0", "tag1", "tag2", "tag3"]
    for (_, got), want in zip(done, sent):
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert ring.out[0].shape == (4, 3) and ring.out[1].shape == (5, 4)
    # a call that left before finish() does not leak its last submission into the next call
    ring.submit(sent[0], None, "stale")
    done.clear()
    ring.start(lambda tag, rows: done.append((tag, rows.copy())))
    ring.submit(sent[1], None, "fresh")
    ring.finish()
    assert [tag for tag, _ in done] == ["fresh"] and np.array_equal(done[0][1], sent[1].numpy())


def test_serial_path_of_the_tile_encoder_on_a_stand_in_engine():
    class TileEngine:  # "embeds" a crop as (its first pixel, its height)
        def __init__(self):
            self.groups, self.threads = [], set()

        def preprocess_tiles(self, pix, offs, hw, tile, max_tiles):
            self.groups.append(len(offs))
            self.threads.add(threading.get_ident())
            return (pix[torch.from_numpy(offs)].float(), torch.from_numpy(hw[:, 0]).float()), None, None, None

        def tile_vit_forward(self, pv, ids, nt, want_bf16=True):
            self.threads.add(threading.get_ident())
            return None, torch.stack(pv, dim=1), None

    emb = E.RegionEmbedder.__new__(E.RegionEmbedder)
    emb.torch, emb.pool_token, emb.encoder = torch, 0, "mllama_tiles"
    emb.devices, emb.device = ["cpu"], CPU
    emb.engines = [TileEngine()]
    emb.engine = emb.engines[0]
    items = [np.full((3 + i, 5, 3), i, dtype=np.uint8) for i in range(70)]
    items[40] = "/nonexistent/region.png"
    out = emb.get_image_embeddings(items)
    assert [v for i, v in enumerate(out) if i != 40] == [[float(i), float(3 + i)] for i in range(70) if i != 40] and out[40] is None
    assert emb.engine.groups == [32, 31, 6] and max(emb.engine.groups) <= emb.TILE_GROUP_CROPS
    assert emb.engine.threads == {threading.get_ident()}
    arr, ok = emb.get_image_embeddings(items[:5], as_array=True)
    assert ok.all() and arr.tolist() == out[:5]
