"""Every asynchronous entry point runs on the caller's stream (include/mme.h, Conventions).

The other GPU tests call the engine on torch's default stream and synchronise the device behind every call: a launcher that
passes 0 for `s`, scratch that two calls in flight share, a caller's host array read after the call returned, or state
initialised on one stream and consumed on another are all invisible there.  Here every public entry point runs under the
probes of tests/stream_probes.py (its docstring says what each one sees): probe A against a busy null stream, probe B behind a
late input, twice back to back without a host synchronise and with the caller's host arrays overwritten on return, and probe C
as an event-ordered chain over three streams.  The reference is the same call on a fresh engine on the default stream between
two device synchronises, compared bit for bit (K14's edge list as a set with its similarities, as tests/test_gpu_duplicates.py
compares it).  A fresh Engine per case: the first-call paths (`ensure`, the zero-bias memset) run under the probe.

Poison and overwrite values are valid inputs of the same shape (indices in range, boxes of the same size, crops that fit the
packed buffer from any of the offsets): a misplaced read gives a wrong answer, never an out-of-range access.

Sharpness: mme_normalise_rows, mme_cosine and mme_preprocess are also called with stream = NULL while the current stream is
the side stream -- what a library that ignores its stream does.  Both probes must report a mismatch and be effective.

Effectiveness: `pytest -s` prints one row per entry point and probe (DESIGN.md has the table).  Asserted: every probed entry point
has at least one effective probe, except those of SYNCHRONOUS below, whose documentation says that they make the host wait.

The delay: in-place negations of a 512 MiB tensor on the chosen stream, calibrated once with events to 140 ms (asserted within
40 .. 200 ms; a tiny forward enqueues about 1.5 ms of launches).  On an MI355X: 790 negations, 140.1 ms.  The side streams are
chosen once (stream_probes.side_streams): the runtime maps streams onto four hardware queues, and a stream that shares the null
stream's queue runs in its order whatever the library does; of four streams tried, three were independent.

Found by the probes: no violation.  What they did show is where the host waits ("Streams"): the
entry points that say so, the chunk loop, and `ensure` when scratch has to grow -- the chunk_2 cases of mixed crop sizes regrow
their tables in the second chunk, which waits for the whole device, so neither probe is effective on them; the same towers at
the default chunk or at chunk 4 are.  `neighbours` in the fused form runs at N = 16384, d = 128, the smallest table that form accepts.

The module: 139 tests in 26 .. 29 s on an MI355X; the slowest case is tile_vit_forward under probe A, 1.0 .. 1.5 s.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import duplicates_reference as DR  # noqa: E402
import page_pairs_reference as PR  # noqa: E402
import cluster_reference as CR  # noqa: E402
import stream_probes as sp  # noqa: E402
import tower_mutants as tm  # noqa: E402
from stream_probes import DEV, Case  # noqa: E402

from multimodal_embeddings_amd import weights as W  # noqa: E402
from multimodal_embeddings_amd._lib import Engine  # noqa: E402
from multimodal_embeddings_amd.staging import packed_layout  # noqa: E402

pytestmark = pytest.mark.gpu

# entry point -> the line that makes the host wait; only entry points that include/mme.h documents as synchronising
SYNCHRONOUS = {
    "nms_boxes": "csrc/capi.hip, mme_nms_boxes: hipStreamSynchronize behind the D2H of keep / keep_count (the results are host data)",
    "cluster_pages": "_lib.py, Engine.cluster_pages: labels.cpu() / k.item() (the results are host data)",
    "load_vit_checkpoint + embed": "csrc/weight_load.hip, the staging upload of mme_load_vit_as: hipStreamSynchronize, then hipFree of the staging buffer "
                                   "(mme.h: synchronises `stream` before returning; the host tensors may be released right after)",
}

_fault = []
RECORD = {}  # (entry point, probe) -> [effective, ...]


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


def _record(entry, probe, effective, label=""):
    RECORD.setdefault((entry, probe), []).append(bool(effective))
    print(f"{label or entry:45s} probe {probe}: the delay was {'still pending' if effective else 'over'} when it mattered")


# ---- towers and engines -------------------------------------------------------------------------------------------------
SMALL = dict(hidden_size=384, num_heads=6, intermediate_size=1536, num_layers=2)
TOWERS = {
    "vit16": ("vit", W.ViTGeometry(**SMALL), 41),
    "vit32": ("vit", W.ViTGeometry(patch_size=32, **SMALL), 42),
    "clip16": ("clip", W.CLIPGeometry(**SMALL), 43),
    "siglip16": ("siglip", W.SiglipGeometry(**SMALL), 44),
    "dinov2": ("dinov2", W.Dinov2Geometry(**SMALL), 45),
}
TEXT = {"clip_text": "load_clip_text", "siglip_text": "load_siglip_text"}


@functools.lru_cache(maxsize=None)
def tower_weights(key):
    kind, geom, seed = TOWERS[key]
    return tm.MAKE[kind](seed, geom)


@functools.lru_cache(maxsize=None)
def text_weights(key):
    return tm.weights_of(key, sharp=False)


@functools.lru_cache(maxsize=None)
def tile_weights():
    return tm.tile_weights(sharp=False)


def engine(tower=None, text=None, tile=False, rule=None, chunk=None, attention=None, profile=False, neighbour=None):
    """-> a setup function: a fresh Engine with these loads and settings"""

    def setup():
        eng = Engine(0)
        if tower:
            kind, geom, _ = TOWERS[tower]
            getattr(eng, tm.LOADER[kind])(tower_weights(tower), geom=geom)
        if text:
            getattr(eng, TEXT[text])(text_weights(text), geom=tm.geom_of(text))
        if tile:
            eng.load_tile_vit(tile_weights(), tm.TILE_GEOM)
        if rule is not None:
            eng.set_resize_rule(rule)
        if chunk is not None:
            eng.set_chunk(chunk)
        if attention is not None:
            eng.set_attention_mode(attention)
        if neighbour is not None:
            eng.set_neighbour_mode(neighbour)
        if profile:
            eng.profile(True)
        torch.cuda.synchronize()
        return eng

    return setup


def _raw(eng, name, *args):
    rc = getattr(eng.lib, name)(eng.h, *args)
    assert rc == 0, f"{name}: {eng.lib.mme_last_error(eng.h).decode()}"


# ---- inputs ------------------------------------------------------------------------------------------------------------
HW = np.array([[224, 224], [37, 300], [300, 41]], dtype=np.int32)  # (h, w): the identity, a wide and a tall crop


@functools.lru_cache(maxsize=None)
def crops(v):
    """Three packed crops.  The overwrite (v = 2) of the host tables: every crop 8 x 8 at offset 0, so that any mixture of old
    and new offsets and sizes stays inside the packed buffer"""
    offs, sizes, total = packed_layout(HW)
    rng = np.random.default_rng(100 + v)
    pix = np.zeros(total, dtype=np.uint8)
    for o, n in zip(offs, sizes):
        pix[o:o + n] = rng.integers(0, 256, int(n), dtype=np.uint8)
    if v == 2:
        return {"pix": torch.from_numpy(pix)}, {"offs": np.zeros(3, dtype=np.int64), "hw": np.full((3, 2), 8, dtype=np.int32)}
    return {"pix": torch.from_numpy(pix)}, {"offs": offs.astype(np.int64), "hw": HW.copy()}


def unit_rows(n, d, seed, dtype=torch.bfloat16):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).to(dtype)


def _with(setup, fn):
    """fn(engine) on a throw-away engine on the default stream, synchronised: inputs that an earlier step of the pipeline makes"""
    eng = setup()
    try:
        torch.cuda.synchronize()
        out = fn(eng)
        torch.cuda.synchronize()
        return out
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def patches(tower, v):
    dev, host = crops(v if v < 2 else 3)
    return {"patches": _with(engine(tower), lambda e: e.preprocess(dev["pix"].to(DEV), host["offs"], host["hw"]).cpu())}, {}


CASES = {}


def add(entry, label, setup, inputs, call, **kw):
    assert label not in CASES
    CASES[label] = Case(entry, label, setup, inputs, call, **kw)


# ---- preprocessing ---------------------------------------------------------------------------------------------------
def call_preprocess(eng, d, h, null=False):
    if not null:
        return {"patches": eng.preprocess(d["pix"], h["offs"], h["hw"])}
    g = eng.vit_geometry()
    out = torch.full((3 * g.num_patches, (g.patch_dim + 63) // 64 * 64), 3.0, dtype=torch.bfloat16, device=DEV)
    _raw(eng, "mme_preprocess", d["pix"].data_ptr(), h["offs"].ctypes.data, h["hw"].ctypes.data, 3, out.data_ptr(), None)
    return {"patches": out}


for rule in ("fit_pad", "clip"):
    for tower, chunk in ((None, None), (None, 2), ("vit32", None), ("dinov2", None)):
        add("preprocess", f"preprocess-{rule}-{tower or 'patch16'}-chunk_{chunk or 'default'}", engine(tower, rule=rule, chunk=chunk), crops, call_preprocess)

add("preprocess_tiles", "preprocess_tiles", engine(), crops,
    lambda eng, d, h: dict(zip(("pv", "ids", "mask", "nt"), eng.preprocess_tiles(d["pix"], h["offs"], h["hw"]))))

PAGE_HW = (200, 300)


@functools.lru_cache(maxsize=None)
def boxes(v):
    """Four boxes, two of them over the page's edge; v moves them and keeps their sizes, so the packed layout is one"""
    page = np.random.default_rng(200 + v).integers(0, 256, PAGE_HW + (3,), dtype=np.uint8)
    b = np.array([[-5, -5, 40, 30], [10, 20, 110, 90], [250, 150, 320, 220], [100, 60, 160, 100]], dtype=np.int32)
    b[:, [0, 2]] += 3 * v
    b[:, [1, 3]] += 2 * v
    offs = packed_layout(np.stack([b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]], axis=1))[0].astype(np.int64)
    return {"page": torch.from_numpy(page)}, {"boxes": b, "offs": offs if v < 2 else np.zeros(4, dtype=np.int64)}


def call_crop_boxes(eng, d, h):
    hw = np.stack([h["boxes"][:, 3] - h["boxes"][:, 1], h["boxes"][:, 2] - h["boxes"][:, 0]], axis=1)
    pix = torch.zeros(packed_layout(hw)[2], dtype=torch.uint8, device=DEV)
    _raw(eng, "mme_crop_boxes", d["page"].data_ptr(), PAGE_HW[0], PAGE_HW[1], h["boxes"].ctypes.data, 4, pix.data_ptr(), h["offs"].ctypes.data, eng._stream())
    return {"pix": pix}


add("crop_boxes", "crop_boxes", engine(), boxes, call_crop_boxes)


@functools.lru_cache(maxsize=None)
def picture(v):
    return {"src": torch.from_numpy(np.random.default_rng(300 + v).integers(0, 256, (131, 97, 3), dtype=np.uint8))}, {}


add("lanczos_resize", "lanczos_resize", engine(), picture, lambda eng, d, h: {"out": eng.lanczos_resize(d["src"], 64, 45)})

# ---- image towers --------------------------------------------------------------------------------------------------------
def call_embed(eng, d, h):
    return dict(zip(("e32", "e16"), eng.embed(d["pix"], h["offs"], h["hw"])))


def call_embed_tokens(eng, d, h):
    return dict(zip(("tokens", "e32", "e16"), eng.embed_tokens(d["pix"], h["offs"], h["hw"])))


def call_vit_forward(eng, d, h):
    return dict(zip(("e32", "e16"), eng.vit_forward(d["patches"])))


def call_vit_tokens(eng, d, h):
    return dict(zip(("tokens", "e32", "e16"), eng.vit_tokens(d["patches"])))


for tower in TOWERS:
    add("embed", f"embed-{tower}", engine(tower), crops, call_embed)
    add("embed", f"embed-{tower}-chunk_2", engine(tower, chunk=2), crops, call_embed)
    add("embed_tokens", f"embed_tokens-{tower}", engine(tower), crops, call_embed_tokens)
    add("vit_forward", f"vit_forward-{tower}-chunk_2", engine(tower, chunk=2), functools.partial(patches, tower), call_vit_forward)
    add("vit_forward", f"vit_forward-{tower}", engine(tower), functools.partial(patches, tower), call_vit_forward)
    add("vit_tokens", f"vit_tokens-{tower}-chunk_2", engine(tower, chunk=2), functools.partial(patches, tower), call_vit_tokens)
add("embed_tokens", "embed_tokens-vit16-chunk_2", engine("vit16", chunk=2), crops, call_embed_tokens)
# one pass and a workspace of four crops: at the default chunk the first call allocates the workspace of 4096 crops (6 GB and
# more), which can outlast the delay, and under chunk 2 the second chunk regrows the preprocessing tables (a device synchronise)
add("embed", "embed-vit16-chunk_4", engine("vit16", chunk=4), crops, call_embed)
add("embed_tokens", "embed_tokens-vit16-chunk_4", engine("vit16", chunk=4), crops, call_embed_tokens)
add("vit_tokens", "vit_tokens-vit16", engine("vit16"), functools.partial(patches, "vit16"), call_vit_tokens)
add("embed", "embed-vit16-attention_mode_2", engine("vit16", attention=2), crops, call_embed)
add("embed", "embed-vit16-profile", engine("vit16", profile=True), crops, call_embed, ref_setup=engine("vit16"))

# ---- text and tile towers --------------------------------------------------------------------------------------------------
LENGTHS = {"clip_text": [[2, 9, 33, 77], [77, 5, 2, 40], [3, 3, 3, 3]], "siglip_text": [[1, 9, 33, 64], [64, 5, 2, 40], [3, 3, 3, 3]]}


@functools.lru_cache(maxsize=None)
def token_ids(key, v):
    if key == "clip_text":
        return {}, {"ids": W.synthetic_token_ids(4, tm.VOCAB, tm.VOCAB - 1, seed=400 + v, lengths=LENGTHS[key][v])}
    return {}, {"ids": W.siglip_token_ids(4, tm.VOCAB, tm.TOWERS[key].geom.pad_token_id, seed=400 + v, lengths=LENGTHS[key][v])}


for key in TEXT:
    add("text_forward", f"text_forward-{key}", engine(text=key), functools.partial(token_ids, key),
        lambda eng, d, h: dict(zip(("e32", "e16"), eng.text_forward(h["ids"]))))


@functools.lru_cache(maxsize=None)
def tiles(v):
    """Two images of 1 and 2 tiles.  The overwrite of the id tables: both exchanged (ids 1..8 and counts 1..4 stay in range; the
    pixel buffer holds four tiles per image whatever the count)"""
    rng = np.random.default_rng(500 + v)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in tm.TILE_IMAGES[:2]]
    hw = np.array([a.shape[:2] for a in images], dtype=np.int32)
    offs, _, total = packed_layout(hw)
    pix = np.zeros(total, dtype=np.uint8)
    for o, a in zip(offs, images):
        pix[o:o + a.size] = a.reshape(-1)
    pv, ids, _, nt = _with(engine(), lambda e: e.preprocess_tiles(torch.from_numpy(pix).to(DEV), offs, hw))
    ids, nt = np.asarray(ids, dtype=np.int32), np.asarray(nt, dtype=np.int32)
    assert nt.tolist() == [1, 2]
    return {"pv": pv.cpu()}, {"ids": ids[::-1].copy() if v == 2 else ids, "nt": nt[::-1].copy() if v == 2 else nt}


add("tile_vit_forward", "tile_vit_forward", engine(tile=True), tiles,
    lambda eng, d, h: dict(zip(("hidden", "e32", "e16"), eng.tile_vit_forward(d["pv"], h["ids"], h["nt"], want_hidden=True))))


# ---- the table side ----------------------------------------------------------------------------------------------------------
def call_normalise(eng, d, h, null=False):
    if not null:
        return {"y": eng.normalise_rows(d["x"])}
    y = torch.full(d["x"].shape, 3.0, dtype=torch.bfloat16, device=DEV)
    _raw(eng, "mme_normalise_rows", d["x"].data_ptr(), d["x"].shape[0], d["x"].shape[1], y.data_ptr(), None)
    return {"y": y}


def call_cosine(eng, d, h, null=False):
    if not null:
        return {"S": eng.cosine(d["a"], d["b"])}
    out = torch.full((130, 260), 3.0, dtype=torch.float32, device=DEV)
    _raw(eng, "mme_cosine", d["a"].data_ptr(), 130, d["b"].data_ptr(), 260, 128, out.data_ptr(), 260, None)
    return {"S": out}


add("normalise_rows", "normalise_rows", engine(),
    lambda v: ({"x": torch.from_numpy(np.random.default_rng(600 + v).standard_normal((300, 768)).astype(np.float32))}, {}), call_normalise)
ab = lambda v: ({"a": unit_rows(130, 128, 610 + v), "b": unit_rows(260, 128, 620 + v)}, {})  # noqa: E731
add("cosine", "cosine", engine(), ab, call_cosine)
add("cosine_bf16", "cosine_bf16", engine(), ab, lambda eng, d, h: {"S": eng.cosine_bf16(d["a"], d["b"])})


def table600(v):
    return {"emb": unit_rows(600, 64, 630 + v), "group": torch.from_numpy(np.random.default_rng(640 + v).integers(0, 40, 600).astype(np.int32))}, {}


add("neighbours", "neighbours-mode_1", engine(neighbour=1), table600,
    lambda eng, d, h: dict(zip(("idx", "sim"), eng.neighbours(d["emb"], d["group"], fetch=30, top_n=10))))


@functools.lru_cache(maxsize=None)
def table16k(v):
    """the smallest table the fused form takes (csrc/capi.hip, mme_neighbours: d >= 128, N / 8 >= 2048, 256 cosine tiles of 256 x 256)"""
    return {"emb": unit_rows(16384, 128, 635 + v), "group": torch.from_numpy(np.random.default_rng(645 + v).integers(0, 400, 16384).astype(np.int32))}, {}


add("neighbours", "neighbours-mode_2", engine(neighbour=2), table16k,
    lambda eng, d, h: dict(zip(("idx", "sim"), eng.neighbours(d["emb"], d["group"], row0=512, nrows=1024, fetch=30, top_n=10))))


@functools.lru_cache(maxsize=None)
def pages(v):
    """The planted table of tests/page_pairs_reference.py under two validity masks; the overwrite of page_offs is another valid
    partition of the same rows"""
    t = PR.table(64)
    rng = np.random.default_rng(650 + v)
    dev = {"emb": torch.from_numpy(t.x).to(torch.bfloat16), "area": torch.from_numpy(np.ascontiguousarray(rng.permutation(t.area))),
           "valid": torch.from_numpy((rng.random(t.N) < 0.8).astype(np.uint8))}
    offs = np.ascontiguousarray(t.offs, dtype=np.int32) if v < 2 else np.linspace(0, t.N, t.P + 1).astype(np.int32)
    return dev, {"page_offs": offs}


add("page_similarity", "page_similarity", engine(), pages,
    lambda eng, d, h: {"S": eng.page_similarity(d["emb"], d["area"], d["valid"], h["page_offs"], max_query=10, top_k=10, max_dist=0.5)})
add("page_similarity_pairs", "page_similarity_pairs", engine(), pages,
    lambda eng, d, h: {"S": eng.page_similarity(d["emb"], d["area"], d["valid"], h["page_offs"], max_query=10, top_k=10, max_dist=0.5, pair_range=(5, 40))})


def call_cluster(eng, d, h):
    labels, k, scores = eng.cluster_pages(d["S"], None, "reference_fallback")
    return {"labels": np.asarray(labels), "k": np.asarray(k), "scores": np.asarray(scores, dtype=np.float64)}


add("cluster_pages", "cluster_pages", engine(), lambda v: ({"S": torch.from_numpy(CR.blocked(33, 660 + v))}, {}), call_cluster)


@functools.lru_cache(maxsize=None)
def walks(v):
    c = DR.case(331, 128, 1 + v, 12)
    return {"emb": c["xb"], "group": torch.from_numpy(c["group"])}, {"tau": np.array([c["tau"]])}


def dup_canon(o):
    """edges[:written] in (i, j) order with their similarities: the order atomics wrote them in is arbitrary"""
    w = int(o["counters"][1])
    e, s = o["edges"][:w], o["edge_sim"][:w]
    order = np.lexsort((e[:, 1], e[:, 0]))
    return {**o, "edges": e[order], "edge_sim": s[order]}


def call_duplicates(eng, d, h):
    """init x 2, a scan of each half into its own state, merge, finish"""
    tau = float(h["tau"][0])
    A, B = eng.duplicates_init(331, pages=12, edge_cap=4096), eng.duplicates_init(331, pages=12)
    eng.duplicates_scan(A, d["emb"], d["group"], d["group"], min_sim=tau, row0=0, nrows=331)
    eng.duplicates_scan(B, d["emb"], d["group"], d["group"], min_sim=tau, row0=150, nrows=181)
    C2 = eng.duplicates_init(331, pages=12)
    eng.duplicates_scan(C2, d["emb"], d["group"], d["group"], min_sim=tau, row0=0, nrows=150)
    eng.duplicates_merge(C2, B)
    merged = eng.duplicates_finish(C2)
    whole = eng.duplicates_finish(A)
    return {**whole, **{"merged_" + k: merged[k] for k in ("labels", "degree", "best_idx", "best_sim", "summary", "page_pairs")}}


add("duplicates", "duplicates-init-scan-merge-finish", engine(), walks, call_duplicates, canon=dup_canon)

KM = ("labels", "sim", "centroids", "counts", "sums", "info", "objective")


def table500(v):
    """rows around five centres, started from five rows; the overwrite of init_rows: five other valid rows"""
    rng = np.random.default_rng(670 + v)
    x = rng.standard_normal((5, 64))[rng.integers(0, 5, 500)] + 0.4 * rng.standard_normal((500, 64))
    x = torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).to(torch.bfloat16)
    labels = torch.from_numpy(rng.integers(0, 5, 500).astype(np.int32))
    return {"emb": x, "labels": labels}, {"init_rows": np.array([[3, 77, 150, 301, 420], [9, 99, 199, 299, 499], [1, 2, 4, 5, 6]][v], dtype=np.int32)}


def call_kmeans(eng, d, h):
    r = eng.kmeans(d["emb"], 5, init_rows=h["init_rows"], max_iter=20)
    return {k: getattr(r, k) for k in KM}


def call_silhouette(eng, d, h):
    r = eng.silhouette(d["emb"], d["labels"], 5, samples=True)
    return {k: getattr(r, k) for k in ("score", "cluster", "info", "sums", "counts", "samples")}


add("kmeans", "kmeans", engine(), table500, call_kmeans)
add("silhouette", "silhouette", engine(), table500, call_silhouette)
add("siglip_scores", "siglip_scores", engine(text="siglip_text"),
    lambda v: ({"cos": torch.from_numpy(np.random.default_rng(680 + v).uniform(-1, 1, (7, 130)).astype(np.float32))}, {}),
    lambda eng, d, h: {"p": eng.siglip_scores(d["cos"])})


@functools.lru_cache(maxsize=None)
def detections(v):
    rng = np.random.default_rng(690 + v)
    xy = rng.uniform(0, 80, (90, 2))
    b = np.concatenate([xy, xy + rng.uniform(5, 40, (90, 2))], axis=1)
    return {}, {"boxes": b, "scores": rng.random(90), "classes": rng.integers(0, 3, 90).astype(np.int32), "page_offs": np.array([0, 40, 40, 90], dtype=np.int32)}


def call_nms(eng, d, h):
    kept = eng.nms_boxes(h["boxes"], h["scores"], h["classes"], h["page_offs"], 0.5)
    return {"count": np.array([len(k) for k in kept]), "kept": np.concatenate(kept)}


add("nms_boxes", "nms_boxes", engine(), detections, call_nms)


def interleaved_inputs(v):
    a, b, c = table600(v)[0], walks(v), table500(v)
    return {"n_emb": a["emb"], "n_group": a["group"], "d_emb": b[0]["emb"], "d_group": b[0]["group"], "k_emb": c[0]["emb"], "k_labels": c[0]["labels"]}, \
        {"tau": b[1]["tau"], "init_rows": c[1]["init_rows"]}


def call_interleaved(eng, d, h):
    """K12 -> K14 scan -> K15 -> K16 -> K14 finish on one stream: the workspace the four share, the label histogram of finish"""
    tau = float(h["tau"][0])
    st = eng.duplicates_init(331, pages=12, edge_cap=4096)
    idx, sim = eng.neighbours(d["n_emb"], d["n_group"], fetch=30, top_n=10)
    eng.duplicates_scan(st, d["d_emb"], d["d_group"], d["d_group"], min_sim=tau)
    km = eng.kmeans(d["k_emb"], 5, init_rows=h["init_rows"], max_iter=20)
    sil = eng.silhouette(d["k_emb"], d["k_labels"], 5, samples=True)
    dup = eng.duplicates_finish(st)
    return {"idx": idx, "sim": sim, **{"km_" + k: getattr(km, k) for k in KM}, "sil_score": sil.score, "sil_samples": sil.samples, "sil_sums": sil.sums, **dup}


add("interleaved K12-K14-K15-K16", "interleaved", engine(), interleaved_inputs, call_interleaved, canon=dup_canon)


# ---- the probes ----------------------------------------------------------------------------------------------------------------
def test_delay_is_calibrated():
    d = sp.delay()
    print(f"delay: {d.iters} negations of {d.buf.numel() * 4 >> 20} MiB, {d.ms:.1f} ms")
    sp.side_streams()
    print(f"side streams: {len(sp._streams)} independent of the null stream, {len(sp._shared)} tried that run in its order")
    assert sp.Delay.MIN_MS <= d.ms <= sp.Delay.MAX_MS


@pytest.mark.parametrize("label", list(CASES))
def test_probe_a_busy_null_stream(label):
    case = CASES[label]
    bad, effective = sp.probe_a(case)
    _record(case.entry, "A", effective, label)
    assert not bad, (label, bad)


@pytest.mark.parametrize("label", list(CASES))
def test_probe_b_late_input_back_to_back(label):
    case = CASES[label]
    bad, effective = sp.probe_b(case)
    _record(case.entry, "B", effective, label)
    assert not bad, (label, bad)


# ---- probe C: ordered chains across three streams, the null stream busy ---------------------------------------------------------
def _chain(steps_of, inputs_of):
    """The chain on the default stream, a device synchronise around each step, then on three streams.  Both runs use the same
    engines, the reference first: the steps share the context's scratch, and a step that has to regrow what an earlier one
    allocated synchronises the device (csrc/capi.hip, ensure), which would end the delay.  First calls are probes A and B's."""
    made = []

    def fresh(setup):
        made.append(setup())
        return made[-1]

    try:
        steps = steps_of(fresh)
        inputs = sp.to_device(inputs_of())
        want = sp.chain_reference(steps, inputs)
        got, effective = sp.chain_c(steps, inputs)
    finally:
        for e in made:
            e.close()
    return [k for k in want if got[k].tobytes() != want[k].tobytes()], effective


def test_probe_c_boxes_to_cosine():
    """crop_boxes -> embed -> normalise_rows -> cosine_bf16, each on the next of three streams behind an event"""

    def steps_of(fresh):
        eng = fresh(engine("vit16"))
        b = boxes(0)[1]
        hw = np.stack([b["boxes"][:, 3] - b["boxes"][:, 1], b["boxes"][:, 2] - b["boxes"][:, 0]], axis=1).astype(np.int32)
        total = packed_layout(hw)[2]  # zeros: the bytes between two crops are nobody's
        return [(eng, lambda e, x: dict(zip(("pix", "offs", "hw"), e.crop_boxes(x["page"], b["boxes"], out=torch.zeros(total, dtype=torch.uint8, device=DEV))))),
                (eng, lambda e, x: {"e32": e.embed(x["pix"], x["offs"], hw, want_bf16=False)[0]}),
                (eng, lambda e, x: {"rows": e.normalise_rows(x["e32"])}),
                (eng, lambda e, x: {"S": e.cosine_bf16(x["rows"])})]

    bad, effective = _chain(steps_of, lambda: boxes(0)[0])
    _record("chain boxes..cosine_bf16", "C", effective)
    assert not bad, bad


def test_probe_c_resize_to_tokens():
    """lanczos_resize -> preprocess -> vit_tokens"""
    hw = np.array([[64, 45]], dtype=np.int32)
    offs = np.zeros(1, dtype=np.int64)

    def steps_of(fresh):
        eng = fresh(engine("vit16"))
        return [(eng, lambda e, x: {"small": e.lanczos_resize(x["src"], 64, 45, out=torch.zeros(64 * 45 * 3 + 16, dtype=torch.uint8, device=DEV)[:64 * 45 * 3])}),
                (eng, lambda e, x: {"patches": e.preprocess(x["small"].reshape(-1), offs, hw)}),
                (eng, lambda e, x: dict(zip(("tokens", "e32", "e16"), e.vit_tokens(x["patches"]))))]

    bad, effective = _chain(steps_of, lambda: picture(0)[0])
    _record("chain resize..vit_tokens", "C", effective)
    assert not bad, bad


# ---- a load followed by a forward on the same side stream ----------------------------------------------------------------------
def test_load_then_embed_on_one_side_stream(tmp_path):
    """load_vit_checkpoint (it takes the stream) and embed behind it with no synchronise between them, the null stream busy"""
    from multimodal_embeddings_amd import checkpoint as ckpt

    kind, geom, _ = TOWERS["vit16"]
    ckpt.save_checkpoint(tmp_path, tower_weights("vit16"), "vit", "bfloat16", geom)
    ck = ckpt.read_checkpoint(tmp_path, "vit")

    def setup():
        eng = Engine(0)
        torch.cuda.synchronize()
        return eng

    def call(eng, d, h):
        eng.load_vit_checkpoint(ck)
        return call_embed(eng, d, h)

    case = Case("load_vit_checkpoint + embed", "load-then-embed", setup, crops, call)
    for name, probe in (("A", sp.probe_a), ("B", sp.probe_b)):  # B loads twice: the second load replaces the first behind a pass in flight
        bad, effective = probe(case)
        _record(case.entry, name, effective)
        assert not bad, (name, bad)


# ---- sharpness: a caller that ignores its stream must be seen by both probes -------------------------------------------------------
@pytest.mark.parametrize("probe", ["A", "B"])
@pytest.mark.parametrize("label,call", [("normalise_rows", call_normalise), ("cosine", call_cosine), ("preprocess-fit_pad-patch16-chunk_default", call_preprocess)])
def test_a_call_on_the_null_stream_is_seen(label, call, probe):
    bad, effective = (sp.probe_a if probe == "A" else sp.probe_b)(CASES[label], functools.partial(call, null=True))
    print(f"{label} with stream = NULL, probe {probe}: differs in {bad}, effective {effective}")
    assert effective, "the delay ran out before the probe looked: the harness is too weak to see a wrong stream"
    assert bad, "a call enqueued on the null stream went unnoticed"


# ---- the effectiveness record (keep last) ----------------------------------------------------------------------------------------
def test_every_entry_point_has_an_effective_probe():
    entries = sorted({c.entry for c in CASES.values()})
    if not all((e, p) in RECORD for e in entries for p in "AB"):
        pytest.fail("the probes above did not all run: the table is incomplete")
    print(f"\n{'entry point':30s} {'probe A':>10s} {'probe B':>10s}")
    rows = sorted({e for e, _ in RECORD})
    for e in rows:
        cell = lambda p: "-" if (e, p) not in RECORD else f"{sum(RECORD[e, p])}/{len(RECORD[e, p])}"  # noqa: E731
        print(f"{e:30s} {cell('A'):>10s} {cell('B'):>10s}" + (f" {cell('C'):>6s}" if (e, "C") in RECORD else ""))
    weak = [e for e in rows if not any(any(v) for (n, _), v in RECORD.items() if n == e) and e not in SYNCHRONOUS]
    assert not weak, f"no effective probe: {weak}"
