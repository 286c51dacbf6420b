"""The 8000-pixel cap on the device (mme_lanczos_resize): every output byte equals Pillow's Image.resize(..., LANCZOS).

Single calls on the shapes of tests/golden/lanczos_cases.json (inputs regenerated from the seed, compared with the recorded
sha256 of Pillow 12.2.0's bytes and with live Pillow when that version is installed), a source inside a larger buffer, the
refusals, and the cap as the embedder and the region processor use it.  No tolerance anywhere."""
import hashlib
import json
import logging
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import lanczos_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(HERE, "golden", "lanczos_cases.json")))
CASES = GOLDEN["cases"]
SENT = 0xA5


def _pillow_or_none(img, nh, nw):
    try:
        import PIL
        from PIL import Image
    except ImportError:
        return None
    if PIL.__version__ != GOLDEN["pillow"]:
        return None
    return np.asarray(Image.fromarray(img).resize((nw, nh), Image.LANCZOS))


@pytest.fixture(scope="module")
def eng():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def embedder():
    from multimodal_embeddings_amd.embedder import RegionEmbedder
    from multimodal_embeddings_amd.weights import VIT_B16

    return RegionEmbedder(encoder="vit", geometry=replace(VIT_B16, num_layers=2))


class Guarded:
    """n bytes at byte offset `lead` of a sentinel-filled device buffer: what a call may write, and what it may not."""

    def __init__(self, torch, n, lead=0, guard=4096):
        self.n, self.lead, self.guard = n, lead, guard
        self.raw = torch.full((guard + lead + n + guard,), SENT, dtype=torch.uint8, device="cuda:0")
        self.view = self.raw[guard + lead : guard + lead + n]

    def around_untouched(self):
        a = self.guard + self.lead
        return bool((self.raw[:a] == SENT).all()) and bool((self.raw[a + self.n :] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


@pytest.mark.parametrize("kind", ["noise", "binary"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_single_call_equals_pillow(eng, case, kind):
    import torch

    h, w, nh, nw = case["h"], case["w"], case["new_h"], case["new_w"]
    img = ref.make_image(case["seed"], h, w, kind)
    dst = Guarded(torch, nh * nw * 3, lead=case["seed"] % 4)  # the packed output starts at any byte
    out = eng.lanczos_resize(torch.from_numpy(img).cuda(), nh, nw, out=dst.view)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (nh, nw, 3)
    assert hashlib.sha256(got.tobytes()).hexdigest() == case["sha256"][kind], f"{case['name']} / {kind}: not Pillow {GOLDEN['pillow']}'s bytes"
    want = _pillow_or_none(img, nh, nw)
    if want is not None:
        assert np.array_equal(got, want), int((got != want).sum())
    assert dst.around_untouched()


def test_source_inside_a_larger_buffer(eng):
    """A box of a page as the source: odd byte address, pitch > 3 w; the page and the bytes around dst stay as they were."""
    import torch

    for (H, W, y0, x0, h, w, nh, nw, lead) in ((80, 333, 3, 7, 61, 301, 23, 131, 1), (9001, 40, 0, 5, 9001, 13, 8000, 11, 3), (40, 9100, 2, 33, 7, 9001, 6, 8000, 2)):
        page = ref.make_image(77, H, W, "noise")
        flat = Guarded(torch, H * W * 3, lead=1)  # the page itself at an odd address
        flat.view.copy_(torch.from_numpy(page.reshape(-1)))
        dpage = flat.view.view(H, W, 3)
        before = flat.raw.clone()
        dst = Guarded(torch, nh * nw * 3, lead=lead)
        out = eng.lanczos_resize(dpage[y0 : y0 + h, x0 : x0 + w], nh, nw, out=dst.view)
        torch.cuda.synchronize()
        want = ref.resize(page[y0 : y0 + h, x0 : x0 + w], nh, nw)
        live = _pillow_or_none(np.ascontiguousarray(page[y0 : y0 + h, x0 : x0 + w]), nh, nw)
        assert live is None or np.array_equal(live, want)
        assert np.array_equal(out.cpu().numpy(), want)
        assert dst.around_untouched() and bool((flat.raw == before).all())


def test_refusals_name_field_value_and_range(eng):
    import ctypes as C

    import torch

    from multimodal_embeddings_amd._lib import MmeError, lanczos_workspace

    src = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda:0")
    dst = Guarded(torch, 64 * 64 * 3)
    work = Guarded(torch, lanczos_workspace(64, 64, 32, 32))
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def call(h, w, nh, nw, pitch=None, s=src.data_ptr(), d=None, wk=None, wb=None):
        rc = eng.lib.mme_lanczos_resize(eng.h, s, 3 * w if pitch is None else pitch, h, w, dst.view.data_ptr() if d is None else d, nh, nw,
                                        work.view.data_ptr() if wk is None else wk, work.n if wb is None else wb, stream)
        return rc, eng.lib.mme_last_error(eng.h).decode()

    for args, words in (((0, 64, 1, 32), ("h = 0", "1..32768")), ((64, 32769, 32, 8000), ("w = 32769", "1..32768")),
                        ((64, 64, 8001, 32), ("new_h = 8001", "1..8000")), ((64, 64, 32, 0), ("new_w = 0", "1..8000")),
                        ((64, 64, 3, 32), ("h / new_h = 64 / 3", "at most 16")), ((64, 64, 32, 2), ("w / new_w = 64 / 2", "at most 16"))):
        rc, err = call(*args)
        assert rc == -1 and all(w in err for w in words), err
    rc, err = call(64, 64, 32, 32, pitch=191)
    assert rc == -1 and "src_pitch_bytes = 191" in err and "192" in err
    rc, err = call(64, 64, 32, 32, s=None)
    assert rc == -1 and "src_dev is null" in err
    rc, err = call(64, 64, 32, 32, wb=work.n - 1)
    assert rc == -1 and f"work_bytes = {work.n - 1}" in err and str(work.n) in err
    torch.cuda.synchronize()
    assert dst.untouched() and work.untouched()
    # the binding validates before calling, with the same words
    with pytest.raises(MmeError, match=r"new_h = 8001; supported 1\.\.8000"):
        eng.lanczos_resize(src, 8001, 32, out=None)
    with pytest.raises(MmeError, match=r"w / new_w = 64 / 2"):
        eng.lanczos_resize(src, 32, 2)
    with pytest.raises(MmeError, match="uint8 CUDA tensor"):
        eng.lanczos_resize(src.float(), 32, 32)
    # and a good call on the same buffers works
    rc, err = call(64, 64, 32, 32)
    torch.cuda.synchronize()
    n_out = 32 * 32 * 3
    assert rc == 0 and bool((dst.view[:n_out] == 0).all()) and bool((dst.view[n_out:] == SENT).all()) and dst.around_untouched() and work.around_untouched()


# ---- through the embedder ------------------------------------------------------------------------------------------------
def _mixed_items(tmp_path, with_rgba=True):
    from PIL import Image

    rng = np.random.default_rng(5)
    png = str(tmp_path / "oversized.png")
    Image.fromarray(rng.integers(0, 256, (12, 8311, 3), dtype=np.uint8)).save(png)
    items = [rng.integers(0, 256, (40, 60, 3), dtype=np.uint8), rng.integers(0, 256, (6, 9000, 3), dtype=np.uint8), png,
             rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), rng.integers(0, 256, (9000, 120, 3), dtype=np.uint8),
             Image.fromarray(rng.integers(0, 256, (30, 8002, 3), dtype=np.uint8))]
    if with_rgba:
        items.append(Image.fromarray(rng.integers(0, 256, (5, 8200, 4), dtype=np.uint8), "RGBA"))
    return items


def _rows(out):
    assert all(r is not None for r in out)
    return np.asarray(out, dtype=np.float32)


def test_embedder_mixed_list_equals_host_cap(embedder, tmp_path):
    from multimodal_embeddings_amd.embedder import _load_rgb

    items = _mixed_items(tmp_path)
    got = _rows(embedder.get_image_embeddings(items))
    want = _rows(embedder.get_image_embeddings([_load_rgb(x) for x in items]))
    assert got.shape == (len(items), embedder.embed_dim) and np.array_equal(got, want)
    # one vector through embed(), an oversized array
    assert np.array_equal(embedder.embed(items[1]), want[1])


def test_embedder_rgb_items_never_reach_pillows_resize(embedder, tmp_path, monkeypatch):
    """With PIL's resize out of order the RGB-only list still returns the same vectors: the cap ran on the device."""
    from PIL import Image

    from multimodal_embeddings_amd.embedder import _load_rgb

    items = _mixed_items(tmp_path, with_rgba=False)
    want = _rows(embedder.get_image_embeddings([_load_rgb(x) for x in items]))

    def broken(self, *a, **k):
        raise RuntimeError("PIL.Image.Image.resize called")

    monkeypatch.setattr(Image.Image, "resize", broken)
    got = embedder.get_image_embeddings(items)
    one = embedder.embed(items[4])
    monkeypatch.undo()
    assert np.array_equal(_rows(got), want) and np.array_equal(one, want[4])


def test_embedder_zero_sized_cap_is_a_hole(embedder, caplog):
    rng = np.random.default_rng(6)
    items = [rng.integers(0, 256, (50, 50, 3), dtype=np.uint8), rng.integers(0, 256, (1, 9000, 3), dtype=np.uint8),
             rng.integers(0, 256, (5, 9000, 3), dtype=np.uint8)]
    with caplog.at_level(logging.ERROR):
        out = embedder.get_image_embeddings(items)
    assert out[1] is None and "height and width must be > 0" in caplog.text
    want = embedder.get_image_embeddings([items[0], items[2]])
    assert out[0] == want[0] and out[2] == want[1]


def test_tile_encoder_serial_path_equals_host_cap():
    """The unpipelined path (mllama_tiles), on a seeded tower of one local and one global layer."""
    from multimodal_embeddings_amd.embedder import RegionEmbedder, _load_rgb
    from multimodal_embeddings_amd.weights import TILE_VIT

    emb = RegionEmbedder(encoder="mllama_tiles", geometry=replace(TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,)))
    rng = np.random.default_rng(8)
    items = [rng.integers(0, 256, (30, 45, 3), dtype=np.uint8), rng.integers(0, 256, (7, 8500, 3), dtype=np.uint8)]
    got = _rows(emb.get_image_embeddings(items))
    want = _rows(emb.get_image_embeddings([_load_rgb(x) for x in items]))
    assert np.array_equal(got, want)


# ---- through the region processor ------------------------------------------------------------------------------------------
def test_region_processor_embeds_an_oversized_box_inside_the_page(embedder, caplog):
    from multimodal_embeddings_amd.embedder import _load_rgb
    from multimodal_embeddings_amd.region_processor import RegionProcessor
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    rng = np.random.default_rng(9)
    pages = {"/p/wide.png": rng.integers(0, 256, (300, 8200, 3), dtype=np.uint8), "/p/a.png": rng.integers(0, 256, (200, 300, 3), dtype=np.uint8),
             "/p/b.png": rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)}

    def regions(boxes, wh):
        return {"boxes": [[float(v) for v in b] for b in boxes], "classes": [0.0] * len(boxes), "class_names": ["plain_text"] * len(boxes),
                "scores": [0.9] * len(boxes), "image_size": {"width": wh[0], "height": wh[1]}}

    wide_boxes = [[10, 20, 250, 180], [0, 100, 8200, 200]]  # an ordinary box and an 8200 x 100 one, both inside the page
    by_path = {"/p/wide.png": regions(wide_boxes, (8200, 300)), "/p/a.png": regions([[5, 5, 105, 85], [50, 60, 290, 190]], (300, 200)),
               "/p/b.png": regions([[0, 0, 90, 120]], (90, 120))}
    order = ["/p/a.png", "/p/wide.png", "/p/b.png"]
    col = RegionCollection()
    with caplog.at_level(logging.ERROR):
        n = RegionProcessor(embedder, col).process_regions(order, regions_by_path=by_path, pages=pages)
    assert n == col.count() == 5 and "Error in batch processing" not in caplog.text
    got = col.get()
    rows = {(m["parent_image_name"], m["region_index"]): np.asarray(e, dtype=np.float32) for m, e in zip(got["metadatas"], got["embeddings"])}
    # the oversized row is what the embedder gives for the capped crop; its neighbour and the other pages are what they are alone
    page = pages["/p/wide.png"]
    want_big = np.asarray(embedder.get_image_embeddings([_load_rgb(np.ascontiguousarray(page[100:200, 0:8200]))])[0], dtype=np.float32)
    assert np.array_equal(rows[("wide.png", 1)], want_big)
    for path in order:
        one = RegionCollection()
        k = RegionProcessor(embedder, one).process_image_regions(path, by_path[path], page=pages[path])
        assert k == len(by_path[path]["boxes"])
        g = one.get()
        for m, e in zip(g["metadatas"], g["embeddings"]):
            assert np.array_equal(rows[(m["parent_image_name"], m["region_index"])], np.asarray(e, dtype=np.float32))
