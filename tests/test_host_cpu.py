"""CPU-side tests: C-ABI exports, host logic of the reference-interface mirrors, sharding (gloo)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def built_lib():
    from multimodal_embeddings_amd.build import build

    return build()


def test_library_exports_every_declared_symbol(built_lib):
    """Every function include/mme.h declares is exported and typed by the ctypes loader."""
    from multimodal_embeddings_amd._lib import EXPORTS, load_library

    hdr = open(os.path.join(ROOT, "include", "mme.h")).read()
    declared = set(re.findall(r"\b(mme_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"mme_ctx"}
    assert declared == set(EXPORTS), declared ^ set(EXPORTS)
    lib = load_library(built_lib)
    for name in declared:
        assert getattr(lib, name) is not None
    from multimodal_embeddings_amd._lib import ABI_VERSION

    # the header, the library and the binding name the same ABI version; the product library is not the diagnostic build
    assert int(re.search(r"#define MME_ABI_VERSION (\d+)", hdr).group(1)) == lib.mme_abi_version() == ABI_VERSION == 2
    assert lib.mme_is_diag_build() == 0
    assert isinstance(lib.mme_last_error(None), bytes)


def test_engine_fails_loudly_without_gpu(built_lib):
    import torch

    from multimodal_embeddings_amd._lib import Engine, MmeError

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(MmeError):
        Engine(0)
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    with pytest.raises(MmeError):
        RegionEmbedder()
    with pytest.raises(MmeError):
        RegionEmbedder(device="cpu")


def test_missing_library_is_an_error(tmp_path):
    from multimodal_embeddings_amd._lib import MmeError, load_library

    with pytest.raises(MmeError, match="no CPU fallback"):
        load_library(str(tmp_path / "libmme.so"))


def test_product_code_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package may import it."""
    pkg = os.path.join(ROOT, "multimodal_embeddings_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_weights_are_deterministic_and_bf16_representable():
    from multimodal_embeddings_amd.weights import make_vit_weights, round_to_bf16, synthetic_crops, vit_tensor_specs

    w = make_vit_weights(seed=1)
    assert len(w) == len(vit_tensor_specs()) == 4 + 12 * 16 + 2
    assert sum(v.size for v in w.values()) == 85_798_656  # ViT-B/16 without pooler
    q = w["layers.3.attention.q_proj.weight"]
    assert np.array_equal(q, round_to_bf16(q))
    assert abs(float(q.std()) - 0.02) < 5e-4 and abs(float(q.mean())) < 1e-4
    # known-answer values: any change of the generator invalidates the committed goldens
    assert q.flat[:3].tolist() == make_vit_weights(seed=1)["layers.3.attention.q_proj.weight"].flat[:3].tolist()
    hf = make_vit_weights(seed=1, trained_like=False)
    assert np.all(hf["layers.0.mlp.fc1.bias"] == 0) and np.all(hf["layernorm.weight"] == 1)
    c = synthetic_crops(3, seed=0)
    assert c.shape == (3, 224, 224, 3) and c.dtype == np.uint8
    assert np.array_equal(synthetic_crops(1, seed=0, start=2)[0], c[2])
    assert 120 < c.mean() < 135


def test_region_collection_and_page_table(golden_dir):
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection, build_page_table, same_prefix_skip

    col = RegionCollection()
    metas = [
        {"parent_image_name": "b.png", "region_type": "title", "area_percentage": 2.0, "is_region": True},
        {"parent_image_name": "a.png", "region_type": "plain_text", "area_percentage": 1.0, "is_region": True},
        {"parent_image_name": "b.png", "region_type": "abandon", "area_percentage": 3.0, "is_region": True},
        {"parent_image_name": "a.png", "region_type": "figure", "area_percentage": 0.0, "is_region": True},
        {"parent_image_name": "zzz.png", "region_type": "figure", "area_percentage": 5.0, "is_region": True},
        {"parent_image_name": "a.png", "region_type": "table", "area_percentage": 4.0, "is_region": False},
    ]
    col.upsert(ids=[f"r{i}" for i in range(6)], embeddings=[[float(i)] * 4 for i in range(6)], metadatas=metas)
    col.upsert(ids=["r1"], embeddings=[[9.0] * 4], metadatas=[metas[1]])  # update in place
    assert col.count() == 6
    got = col.get(include=["metadatas", "embeddings"], where={"is_region": {"$eq": True}})
    assert got["ids"] == ["r0", "r1", "r2", "r3", "r4"]
    emb, area, valid, offs = build_page_table(got, ["a.png", "b.png", "c.png"])
    assert offs.tolist() == [0, 2, 4, 4]  # page order of image_paths, collection order inside a page, zzz dropped
    assert emb[:, 0].tolist() == [9.0, 3.0, 0.0, 2.0]
    assert area.tolist() == [1.0, 0.0, 2.0, 3.0]
    assert valid.tolist() == [1, 0, 1, 0]  # zero area and foreign type are invalid (wrc:136)
    names = ["Atlanta GA Atlanta Constitution 1.png", "Atlanta GA Atlanta Constitution 2.png", "Short.png", "Short.png2"]
    sk = same_prefix_skip(names)
    assert sk[0, 1] == 1 and sk[0, 2] == 0 and sk[2, 3] == 0 and sk[2, 2] == 1
    assert same_prefix_skip(names, 5)[2, 3] == 1


def test_compute_image_similarity_matrix_empty_collection():
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection, compute_image_similarity_matrix

    assert compute_image_similarity_matrix(RegionCollection(), ["/x/a.png"]) == (None, None)


def test_cluster_images_validation_returns_none():
    from multimodal_embeddings_amd.weighted_region_clustering import cluster_images

    assert cluster_images(np.zeros((0, 0)), []) is None
    assert cluster_images(np.zeros((2, 3)), ["a", "b"]) is None
    bad = np.eye(3)
    bad[0, 1] = np.nan
    assert cluster_images(bad, ["a", "b", "c"]) is None
    assert cluster_images([[1.0]], ["a"]) is None


def test_get_image_embeddings_contract_without_gpu_work(monkeypatch):
    """List-in/list-out rules of embedder.py:141-226 that need no device."""
    from multimodal_embeddings_amd import embedder as E

    import threading

    import torch

    class FakeEngine:  # stands in for a device context: "embeds" a crop as (its first pixel, its height, context id)
        def __init__(self, ident, fail_on=None):
            self.ident, self.calls, self.threads, self.fail_on = ident, [], set(), fail_on

        def embed(self, pix, offs, hw, pool_token, want_f32=True, want_bf16=True):
            self.calls.append(len(offs))
            self.threads.add(threading.get_ident())
            if self.fail_on is not None and self.fail_on in hw[:, 0].tolist():
                raise E.MmeError("out of memory (simulated)")
            first = pix[torch.from_numpy(offs)].float()
            return torch.stack([first, torch.from_numpy(hw[:, 0]).float(), torch.full((len(offs),), float(self.ident))], dim=1), None

    def make(n_dev, fail_on=None):
        emb = E.RegionEmbedder.__new__(E.RegionEmbedder)
        emb.torch, emb.pool_token, emb.encoder = torch, 0, "vit_b16"
        emb.devices = ["cpu"] * n_dev
        emb.device = torch.device("cpu")
        emb.engines = [FakeEngine(d, fail_on) for d in range(n_dev)]
        emb.engine = emb.engines[0]
        return emb

    emb = make(1)
    assert emb.get_image_embeddings([]) == []
    assert emb.get_image_embeddings(["/nonexistent/a.png", "/nonexistent/b.png"]) == [None, None]  # None holes, no raise
    with pytest.raises(NotImplementedError):
        emb.get_text_embeddings("Hoosier. Hockey.")
    assert E.MmE5MllamaEmbedder is E.RegionEmbedder
    # fan-out of embedder.py:191-224: item i -> context i % n_devices, one thread per context, order kept
    items = [np.full((10 + i, 7, 3), i, dtype=np.uint8) for i in range(50)]
    items[13] = "/nonexistent/region.png"
    emb = make(3)
    out = emb.get_image_embeddings(items)
    assert out[13] is None and sum(v is None for v in out) == 1
    for i, v in enumerate(out):
        if v is not None:
            assert v == [float(i), float(10 + i), float(i % 3)]
    # every context is driven by ONE thread (a context is not thread-safe); a pool worker that finishes its share early
    # may take the next one, so the number of distinct threads is 2 or 3
    assert all(len(e.threads) == 1 for e in emb.engines) and len(set().union(*(e.threads for e in emb.engines))) >= 2
    arr, ok = emb.get_image_embeddings(items, as_array=True)  # the ndarray form: same rows, a mask instead of None holes
    assert arr.shape == (50, 3) and ok.tolist() == [i != 13 for i in range(50)]
    assert all(arr[i].tolist() == out[i] for i in range(50) if i != 13) and not arr[13].any()
    # a single query image takes the first context (embedder.py:158-185)
    assert emb.get_image_embeddings([items[5]], is_query=True)[0][2] == 0.0
    # batch_size bounds a device pass (16 crops per unit) ...
    emb = make(1)
    emb.get_image_embeddings(items[:12] + items[14:], batch_size=1)
    assert emb.engines[0].calls == [16, 16, 16]
    # ... and so does the byte budget
    emb = make(1)
    emb.GROUP_BYTES = 3 * 7 * 3 * 14
    emb.get_image_embeddings(items[:6])
    assert sum(emb.engines[0].calls) == 6 and len(emb.engines[0].calls) >= 2
    # a failing pass voids only its own group (the reference isolates failures per image, embedder.py:135-137)
    emb = make(1, fail_on=10 + 20)
    out = emb.get_image_embeddings(items[:12] + items[14:], batch_size=1)
    assert [v is None for v in out] == [False] * 16 + [True] * 16 + [False] * 16


def test_load_rgb_rules(golden_dir):
    from PIL import Image

    from multimodal_embeddings_amd.embedder import _load_rgb

    f = os.path.join(golden_dir, "crops", json.load(open(os.path.join(golden_dir, "crops_manifest.json")))["crops"][0]["file"])
    a = _load_rgb(f)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
    assert np.array_equal(a, _load_rgb(Image.open(f)))
    assert np.array_equal(a, _load_rgb(a))
    big = np.zeros((10, 9000, 3), dtype=np.uint8)  # > 8000 px: LANCZOS cap (embedder.py:110-114)
    assert _load_rgb(big).shape == (int(10 * 8000 / 9000), 8000, 3)
    with pytest.raises(ValueError):
        _load_rgb(np.zeros((4, 4), dtype=np.uint8))


def test_last_pooling_mirror_matches_reference_golden(golden_dir):
    import torch

    from multimodal_embeddings_amd.embedder import last_pooling

    g = np.load(os.path.join(golden_dir, "last_pooling.npz"))
    out = last_pooling(torch.from_numpy(g["hs"]), torch.from_numpy(g["mask"]))
    assert np.array_equal(out.numpy(), g["out"])


def test_shard_helpers():
    from multimodal_embeddings_amd.dist import shard_pages, shard_range

    for n, w in [(10, 3), (4096, 8), (7, 8), (0, 2), (65536, 8)]:
        parts = [shard_range(n, r, w) for r in range(w)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1
    offs = np.array([0, 10, 10, 50, 60, 100, 130])
    parts = [shard_pages(offs, r, 3) for r in range(3)]
    assert parts[0][0] == 0 and parts[-1][1] == 6
    assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))


_GLOO_WORKER = r"""
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["MME_ROOT"])
from multimodal_embeddings_amd import dist as mdist
rank, world, local = mdist.init_from_env("gloo")
assert world == 2
# ragged bf16 shards: rank 0 holds rows 0..4, rank 1 rows 5..7
full = (torch.arange(8 * 64, dtype=torch.float32).reshape(8, 64) / 64).to(torch.bfloat16)
a, b = mdist.shard_range(8, rank, world)
counts = [mdist.shard_range(8, r, world)[1] - mdist.shard_range(8, r, world)[0] for r in range(world)]
got = mdist.all_gather_rows(full[a:b].clone(), counts)
assert got.dtype == torch.bfloat16 and torch.equal(got, full), "ragged gather"
even = mdist.all_gather_rows(full[rank * 4:(rank + 1) * 4].clone())
assert torch.equal(even, full), "even gather"
f32 = mdist.all_gather_rows(full.float()[rank * 4:(rank + 1) * 4].clone())
assert torch.equal(f32, full.float())
# gather straight into the head of a resident table (bench.py: rows past the gathered shards stay untouched)
table = torch.full((12, 64), 7.0, dtype=torch.bfloat16)
ret = mdist.all_gather_rows(full[rank * 4:(rank + 1) * 4].clone(), out=table[:8])
assert ret.data_ptr() == table.data_ptr() and torch.equal(table[:8], full) and bool((table[8:] == 7).all()), "gather into out"
rag = torch.zeros(8, 64, dtype=torch.bfloat16)
mdist.all_gather_rows(full[a:b].clone(), counts, out=rag)
assert torch.equal(rag, full), "ragged gather into out"
assert mdist.all_gather_floats(1.5 + rank) == [1.5, 2.5]
# row-block cosine of the gathered matrix equals the single-process result
e = torch.nn.functional.normalize(torch.randn(8, 64, generator=torch.Generator().manual_seed(0)), dim=1)
allv = mdist.all_gather_rows(e[rank * 4:(rank + 1) * 4].clone())
block = e[rank * 4:(rank + 1) * 4] @ allv.T
assert torch.allclose(block, (e @ e.T)[rank * 4:(rank + 1) * 4])
m = mdist.all_reduce_max_float(float(rank + 1))
assert m == 2.0
# ragged int32 / f32 tables (the neighbour lists of K12) gather like the embeddings
tab = torch.arange(8 * 3, dtype=torch.int32).reshape(8, 3)
assert torch.equal(mdist.all_gather_rows(tab[a:b].clone(), counts), tab)
# page-matrix shards: disjoint partial matrices add up exactly; the normalisation is wrc:246-252
P = 7
raw = torch.rand(P, P, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
raw = torch.triu(raw, 1); raw = raw + raw.T
pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
lo, hi = mdist.shard_range(len(pairs), rank, world)
part = torch.zeros_like(raw)
for i, j in pairs[lo:hi]:
    part[i, j] = part[j, i] = raw[i, j]
tot = mdist.all_reduce_sum(part)
assert torch.equal(tot, raw), "shard sum"
S = mdist.normalise_page_matrix(tot)
off = raw[~torch.eye(P, dtype=torch.bool)]
assert torch.equal(torch.diagonal(S), torch.ones(P, dtype=torch.float64)) and S[0, 1] == raw[0, 1] / off.max() and S.max() == 1.0
assert torch.equal(mdist.normalise_page_matrix(torch.zeros(3, 3, dtype=torch.float64)), torch.eye(3, dtype=torch.float64))
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_all_gather_rows_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ, MME_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29731", WORLD_SIZE="2", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "ok" in o


_FORCED_WORKER = r"""
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["MME_ROOT"])
from multimodal_embeddings_amd import dist as mdist
assert not mdist.collectives_active()
rank, world, local = mdist.init_from_env("gloo", force=True)
assert (rank, world) == (0, 1) and dist.is_initialized() and mdist.collectives_active()
calls = []
real = dist.all_gather_into_tensor
dist.all_gather_into_tensor = lambda out, inp, **kw: (calls.append(tuple(out.shape)), real(out, inp, **kw))[1]
full = (torch.arange(8 * 64, dtype=torch.float32).reshape(8, 64) / 64).to(torch.bfloat16)
table = torch.full((12, 64), 7.0, dtype=torch.bfloat16)
mdist.all_gather_rows(full.clone(), out=table[:8])
assert calls == [(8, 128)], calls  # the collective really ran, on the byte view of the table slice
assert torch.equal(table[:8], full) and bool((table[8:] == 7).all())
assert mdist.all_gather_floats(2.5) == [2.5] and len(calls) == 2
t = torch.ones(3, 3, dtype=torch.float64)
assert torch.equal(mdist.all_reduce_sum(t), torch.ones(3, 3, dtype=torch.float64))
dist.barrier(); dist.destroy_process_group()
print("forced ok")
"""


def test_forced_process_group_of_one_rank_runs_the_collectives(tmp_path):
    """`init_from_env(force=True)` (bench.py --force-dist): at WORLD_SIZE = 1 the process group exists and every helper
    of dist.py goes through it -- the rehearsal the GPU box runs on nccl (tests/test_gpu_dist.py), here on gloo."""
    script = tmp_path / "forced.py"
    script.write_text(_FORCED_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MME_FORCE_DIST")}
    env.update(MME_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29741", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "forced ok" in r.stdout, r.stdout + r.stderr


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` without a launcher must start 2 rank processes itself, before anything touches a GPU
    (VERDICT r1 #1): the launcher half is exercised here with the rank body replaced by an environment echo."""
    sys.path.insert(0, ROOT)
    import bench

    probe = tmp_path / "probe.py"
    probe.write_text("import os, sys\nprint('rank', os.environ['RANK'], os.environ['LOCAL_RANK'], os.environ['WORLD_SIZE'], "
                     "os.environ['MASTER_ADDR'], 'torch' in sys.modules, sys.argv[1:], flush=True)\n"
                     "print('{\"json\": ' + os.environ['RANK'] + '}', flush=True)\n"
                     "sys.exit(3 if os.environ['RANK'] == '1' and '--fail' in sys.argv else 0)\n")
    code = ("import sys; sys.path.insert(0, %r); import bench; bench.__file__ = %r; "
            "assert 'torch' not in sys.modules; sys.exit(bench.launch_ranks(2, sys.argv[1:]))" % (ROOT, str(probe)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, "-c", code, "--steps", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == '{"json": 0}'  # only rank 0's JSON line reaches stdout ...
    assert "rank 0 0 2 127.0.0.1 False ['--steps', '1']" in r.stderr  # ... its chatter ...
    assert "rank 1 1 2 127.0.0.1 False ['--steps', '1']" in r.stderr and '{"json": 1}' in r.stderr  # ... and the other ranks go to stderr
    r = subprocess.run([sys.executable, "-c", code, "--fail"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 3  # a failing rank fails the launch
    a = bench.parse_args(["--gpus", "8"])
    assert a.gpus == 8 and a.config == "auto" and a.steps == 5 and a.timeout > 0


def test_bench_launcher_fails_fast_when_a_rank_dies(tmp_path):
    """a rank != 0 that dies mid-run must not leave the parent blocked on rank 0's stdout while rank 0
    sits in a collective: the launcher polls every rank, stops the rest and returns non-zero within seconds; a run
    that never ends is bounded by --timeout."""
    import time

    probe = tmp_path / "probe.py"
    # rank 0 "hangs in the collective" (sleeps far longer than the test allows); rank 1 dies after it has started
    probe.write_text("import os, sys, time, signal\n"
                     "print('started', os.environ['RANK'], flush=True)\n"
                     "if os.environ['RANK'] == '1' and '--die' in sys.argv:\n"
                     "    time.sleep(0.5); os.kill(os.getpid(), signal.SIGKILL)\n"
                     "time.sleep(600)\n")
    code = ("import sys; sys.path.insert(0, %r); import bench; bench.__file__ = %r; "
            "sys.exit(bench.launch_ranks(2, sys.argv[2:], float(sys.argv[1])))" % (ROOT, str(probe)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code, "0", "--die"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 137, (r.returncode, r.stderr)  # SIGKILL of rank 1, reported the shell's way
    assert time.monotonic() - t0 < 15.0
    assert "rank 1 exited" in r.stderr
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code, "1.5"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 124 and time.monotonic() - t0 < 15.0, (r.returncode, r.stderr)


def test_graft_entry_build():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g

    g.build()


def test_region_rows_mirror_matches_reference_rows(golden_dir):
    """multimodal_embeddings_amd.region_processor.region_rows == the rows the reference's RegionProcessor upserted."""
    import json

    from multimodal_embeddings_amd.region_processor import load_region_cache, region_rows

    g = json.load(open(os.path.join(golden_dir, "region_rows.json")))
    ids, metas, boxes = region_rows("<page_path>/" + g["page_name"], g["regions"])
    assert ids == g["ids"]
    assert [dict(m, parent_image="<page_path>") for m in metas] == g["metadatas"]
    assert boxes.dtype == np.int32 and boxes.tolist()[3] == [-3, 100, 40, 130]  # int() truncates toward zero
    assert [[int(b[3] - b[1]), int(b[2] - b[0]), 3] for b in boxes] == g["crop_shapes"]
    # cache schema of doclayout_detector.py:145-153
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        pth = os.path.join(d, "x_conf0.1_iou0.45.json")
        json.dump(g["regions"], open(pth, "w"))
        assert load_region_cache(pth)["image_size"] == {"width": 300, "height": 220}


def test_store_round_trip_and_progress_log(tmp_path):
    """Region rows survive save/load in order and value; the resume log is idempotent, append-only and
    reads the reference's `{"completed_...": [...]}` progress files."""
    import json

    from multimodal_embeddings_amd.store import ProgressLog, load_collection, save_clustering_outputs, save_collection
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    rng = np.random.default_rng(0)
    col = RegionCollection()
    ids = [f"region_p{i // 3}_{i}" for i in range(7)]
    metas = [{"parent_image_name": f"p{i // 3}.png", "region_type": "title", "area_percentage": float(i), "is_region": True} for i in range(7)]
    emb = rng.standard_normal((7, 8)).astype(np.float32)
    col.upsert(ids=ids, embeddings=emb.tolist(), documents=[f"Region: title from p{i // 3}.png" for i in range(7)], metadatas=metas)
    assert save_collection(col, str(tmp_path / "db" / "regions")) == 7
    back = load_collection(str(tmp_path / "db" / "regions")).get(include=["metadatas", "embeddings", "documents"])
    assert back["ids"] == ids and back["metadatas"] == metas and back["documents"][0] == "Region: title from p0.png"
    assert np.array_equal(np.asarray(back["embeddings"], dtype=np.float32), emb)

    S = np.array([[1.0, 0.25], [0.25, 1.0]])
    res = {"n_clusters": 2, "clusters": {"0": ["a.png"], "1": ["b.png"]}, "cluster_cohesion": {0: 0.0, 1: 0.0}, "labels": [0, 1]}
    save_clustering_outputs(str(tmp_path / "out"), S, ["a.png", "b.png"], res)
    assert np.array_equal(np.load(tmp_path / "out" / "similarity_matrix.npy"), S)
    assert json.load(open(tmp_path / "out" / "image_names.json")) == ["a.png", "b.png"]
    saved = json.load(open(tmp_path / "out" / "clustering_results.json"))
    assert saved["cluster_cohesion"] == {"0": 0.0, "1": 0.0} and saved["labels"] == [0, 1]  # int keys -> strings, as wrc:888-889 writes

    log = ProgressLog(str(tmp_path / "progress" / "regions.jsonl"))
    assert not log.done("region_a")
    log.mark("region_a")
    log.mark("region_a")
    log.mark("region_b")
    assert open(log.path).read().count("\n") == 2  # one line per item, no rewrites
    ref = tmp_path / "region_embedding_progress.json"
    json.dump({"completed_regions": ["region_b", "region_c"]}, open(ref, "w"))
    log.import_reference(str(ref), "completed_regions")
    again = ProgressLog(log.path)
    assert len(again) == 3 and again.done("region_c") and not again.done("region_d")


def test_convert_to_rgb_composites_over_white_like_the_mllama_processor():
    """RGBA / LA / palette+transparency crops: `_load_rgb` must hand K1 the pixels transformers' Mllama processor
    would resize (white compositing, image_processing_pil_mllama.py:196-211), not a plain .convert("RGB")."""
    from PIL import Image
    from transformers.models.mllama.image_processing_pil_mllama import convert_to_rgb as hf_convert

    from multimodal_embeddings_amd.embedder import _load_rgb, convert_to_rgb

    rng = np.random.default_rng(11)
    rgba = Image.fromarray(rng.integers(0, 256, (37, 53, 4), dtype=np.uint8), "RGBA")
    la = Image.fromarray(rng.integers(0, 256, (21, 40, 2), dtype=np.uint8), "LA")
    pal = Image.fromarray(rng.integers(0, 256, (30, 30, 3), dtype=np.uint8), "RGB").quantize(16)
    pal.info["transparency"] = 3
    grey = Image.fromarray(rng.integers(0, 256, (19, 23), dtype=np.uint8), "L")
    differs = 0
    for im in (rgba, la, pal, grey):
        want = np.asarray(hf_convert(im))
        assert np.array_equal(np.asarray(convert_to_rgb(im)), want)
        assert np.array_equal(_load_rgb(im), want)
        differs += int(not np.array_equal(want, np.asarray(im.convert("RGB"))))
    assert differs >= 2  # the transparent inputs really exercise the compositing
    rgb = Image.fromarray(rng.integers(0, 256, (8, 9, 3), dtype=np.uint8), "RGB")
    assert convert_to_rgb(rgb) is rgb


def test_collection_update_and_modify():
    """The rest of the collection contract of SURVEY.md 8b: `update` (image_processor.py:219-224) changes fields of existing
    rows only, `modify` / `.metadata` carry the collection-level settings as db_operations.py:50-52 reads and writes them."""
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection

    col = RegionCollection()
    col.upsert(ids=["a", "b"], embeddings=[[1.0, 0.0], [0.0, 1.0]], metadatas=[{"k": 1}, {"k": 2}], documents=["da", "db"])
    col.update(ids=["b", "zzz"], metadatas=[{"k": 3}, {"k": 9}])
    got = col.get(ids=["a", "b"])
    assert got["metadatas"] == [{"k": 1}, {"k": 3}] and got["documents"] == ["da", "db"] and got["embeddings"][1] == [0.0, 1.0]
    assert col.count() == 2  # the unknown id was not added
    col.update(ids=["a"], embeddings=[[0.5, 0.5]])
    assert col.get(ids=["a"])["embeddings"] == [[0.5, 0.5]]
    current = col.metadata or {}
    col.modify(metadata={**current, "hnsw_M": "32", "hnsw_ef": "200"})  # the call db_operations.py:50-52 makes
    assert col.metadata["hnsw_M"] == "32" and col.metadata["hnsw_space"] == "cosine"


def test_collection_where_filters_and_query_shape_without_gpu():
    """chroma-shaped `where` handling of RegionCollection (the filter of every reference call site is {"key": {"$eq": v}})."""
    from multimodal_embeddings_amd.weighted_region_clustering import RegionCollection, _where_mask

    metas = [{"p": "a", "is_region": True}, {"p": "b", "is_region": False}, None, {"p": "a"}]
    assert _where_mask(metas, None) == [True] * 4
    assert _where_mask(metas, {"p": {"$eq": "a"}}) == [True, False, False, True]
    assert _where_mask(metas, {"p": "b"}) == [False, True, False, False]
    assert _where_mask(metas, {"is_region": {"$ne": True}}) == [False, True, False, True]
    assert _where_mask(metas, {"$and": [{"p": {"$eq": "a"}}, {"is_region": {"$eq": True}}]}) == [True, False, False, False]
    assert _where_mask(metas, {"$or": [{"p": {"$eq": "b"}}, {"is_region": {"$eq": True}}]}) == [True, True, False, False]
    with pytest.raises(ValueError):
        _where_mask(metas, {"p": {"$gt": 1}})
    col = RegionCollection()
    col.upsert(ids=["x", "y"], embeddings=[[1.0] * 64, [0.5] * 64], metadatas=[{"p": "a"}, {"p": "b"}])
    assert col.get(where={"p": {"$eq": "b"}})["ids"] == ["y"] and col.count() == 2
    empty = col.query(query_embeddings=[[1.0] * 64], n_results=5, where={"p": {"$eq": "zzz"}})  # nothing to rank: no GPU touched
    assert empty["ids"] == [[]] and empty["distances"] == [[]] and empty["metadatas"] == [[]]
    with pytest.raises(ValueError):
        col.query(n_results=3)
    with pytest.raises(ValueError):
        RegionCollection(metric="manhattan")


def test_create_cross_comparison_host_logic_equals_the_reference_picks_exactly(golden_dir, tmp_path):
    """The walk of `create_cross_comparison` (cross_compare.py:19-283) over an exact f64 brute-force store (a stand-in
    with chroma's get / query / add shapes, no GPU): the picks and the printed 4-decimal distances the REAL function
    produced on that store (neighbour_cases.npz) are reproduced exactly."""
    import json

    from multimodal_embeddings_amd.cross_compare import create_cross_comparison

    g = np.load(os.path.join(golden_dir, "neighbour_cases.npz"))
    names = json.load(open(os.path.join(golden_dir, "neighbour_names.json")))["image_names"]
    emb = g["image_emb"].astype(np.float64)
    paths = [str(tmp_path / nm) for nm in names]
    for p in paths:
        open(p, "w").close()

    class Store:
        ids = [f"image_{nm}" for nm in names]
        metas = [{"image_path": p} for p in paths]

        def get(self, ids=None, include=None, where=None):
            rows = [self.ids.index(i) for i in ids if i in self.ids]
            return {"ids": [self.ids[r] for r in rows], "embeddings": [emb[r].tolist() for r in rows]}

        def query(self, query_embeddings, n_results, include=None, where=None):
            out = {"ids": [], "distances": [], "metadatas": []}
            for q in query_embeddings:
                d = 1.0 - emb @ np.asarray(q, dtype=np.float64)
                order = np.argsort(d, kind="stable")[:n_results]
                out["ids"].append([self.ids[r] for r in order])
                out["distances"].append([float(d[r]) for r in order])
                out["metadatas"].append([self.metas[r] for r in order])
            return out

    rep = create_cross_comparison(None, Store(), paths, query_batch=7)
    assert [p["image"] for p in rep] == names
    for r, page in enumerate(rep):
        want = [int(c) for c in g["image_idx"][r] if c >= 0]
        assert [names.index(s["filename"]) for s in page["similar"]] == want
        assert [f"{s['score']:.4f}" for s in page["similar"]] == [f"{d:.4f}" for d in g["image_distance_4dp"][r][: len(want)]]
    # a path that is not in the store and cannot be embedded (no embedder) is skipped, as :94-106
    assert create_cross_comparison(None, Store(), [str(tmp_path / "ghost.png")]) == []


def test_process_regions_wave_logic_without_a_device():
    """Host side of RegionProcessor.process_regions (region_processor.py:36-60 mirror) with a stand-in engine on CPU
    tensors: waves close at WAVE_CROPS / WAVE_BYTES, rows reach the store per page in page order and in chunks of
    REGION_BATCH_SIZE, a failing device pass voids exactly the pages it carried, a page whose boxes cannot be cut fails
    alone, unreadable and region-less pages are skipped."""
    import torch

    from multimodal_embeddings_amd import config
    from multimodal_embeddings_amd._lib import MmeError
    from multimodal_embeddings_amd.region_processor import RegionProcessor

    import threading

    engine_threads = set()  # every engine call belongs to the thread that called process_regions

    class FakeEngine:
        device = 0

        def crop_boxes(self, page, boxes, out=None, base=0):
            engine_threads.add(threading.get_ident())
            b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
            hw = np.stack([b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]], axis=1).astype(np.int32)
            if hw.max() > 100:
                raise MmeError("box too large (simulated)")
            size = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
            offs = np.zeros(len(b), dtype=np.int64)
            offs[1:] = np.cumsum((size[:-1] + 15) // 16 * 16)
            offs += base
            for (x0, y0, x1, y1), o, sz in zip(b, offs, size):
                out[o : o + sz] = page[y0:y1, x0:x1].reshape(-1)
            return out, offs, hw

    _torch = torch

    class FakeEmbedder:
        torch = _torch
        device = _torch.device("cpu")
        engine = FakeEngine()
        passes = []
        fail_pass = None

        def embed_packed(self, pix, offs, hw, want_bf16=False):
            engine_threads.add(threading.get_ident())
            self.passes.append(len(offs))
            if self.fail_pass is not None and len(self.passes) - 1 == self.fail_pass:
                raise MmeError("out of memory (simulated)")
            first = pix[torch.from_numpy(offs)].float()  # "embedding" = (first byte of the crop, height, width)
            return torch.stack([first, torch.from_numpy(hw[:, 0]).float(), torch.from_numpy(hw[:, 1]).float()], dim=1), None

    class Store:
        def __init__(self):
            self.rows, self.calls = [], []

        def upsert(self, ids, embeddings, documents=None, metadatas=None):
            self.calls.append((metadatas[0]["parent_image_name"], len(ids)))
            self.rows += list(zip(ids, embeddings))

    rng = np.random.default_rng(0)

    def make_page(k, n):
        page = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
        boxes = []
        for _ in range(n):
            x0, y0 = int(rng.integers(0, 100)), int(rng.integers(0, 80))
            boxes.append([x0 + 0.3, y0 + 0.7, x0 + int(rng.integers(2, 50)) + 0.9, y0 + int(rng.integers(2, 30)) + 0.2])
        regions = {"boxes": boxes, "classes": [1.0] * n, "class_names": ["plain_text"] * n, "scores": [0.5] * n, "image_size": {"width": 160, "height": 120}}
        return f"/pages/page {k:02d}.png", page, regions

    specs = [make_page(k, n) for k, n in enumerate([60, 5, 70, 3, 130, 8])]
    pages = {p: a for p, a, _ in specs}
    regs = {p: r for p, _, r in specs}
    regs["/pages/none.png"] = {"boxes": []}
    pages["/pages/none.png"] = np.zeros((8, 8, 3), np.uint8)
    regs["/pages/big.png"] = {"boxes": [[0, 0, 150, 10]], "classes": [1.0], "class_names": ["title"], "scores": [1.0], "image_size": {"width": 160, "height": 120}}
    pages["/pages/big.png"] = np.zeros((120, 160, 3), np.uint8)
    order = [specs[0][0], "/pages/missing.png", specs[1][0], "/pages/none.png", specs[2][0], "/pages/big.png", specs[3][0], specs[4][0], specs[5][0]]
    regs["/pages/missing.png"] = specs[0][2]  # regions known, pixels unreadable

    def run(fail_pass=None, wave=64):
        emb, store = FakeEmbedder(), Store()
        emb.passes, emb.fail_pass = [], fail_pass
        rp = RegionProcessor(emb, store)
        rp.WAVE_CROPS = wave
        n = rp.process_regions(order, regions_by_path=regs, pages=pages)
        return n, emb, store

    n, emb, store = run()
    assert n == 60 + 5 + 70 + 3 + 130 + 8 == len(store.rows)
    assert emb.passes == [65, 70, 133, 8]  # waves close once >= 64 crops are in, whole pages only
    assert [c for c in store.calls if c[0] == "page 04.png"] == [("page 04.png", 48), ("page 04.png", 48), ("page 04.png", 34)]
    names = [c[0] for c in store.calls]
    assert sorted(set(names), key=names.index) == [os.path.basename(s[0]) for s in specs]  # page order, big / none / missing absent
    # every row is the crop the reference's int() rule cuts: first byte, height, width
    k = 0
    for path, page, r in specs:
        for i, box in enumerate(r["boxes"]):
            x0, y0, x1, y1 = map(int, box)
            rid, vec = store.rows[k]
            assert rid == f"region_{os.path.splitext(os.path.basename(path))[0]}_{i}" and vec == [float(page[y0, x0, 0]), float(y1 - y0), float(x1 - x0)]
            k += 1
    assert all(cnt <= config.REGION_BATCH_SIZE for _, cnt in store.calls)
    # the second device pass fails: exactly its page (page 02) is missing, everything else arrives
    n2, emb2, store2 = run(fail_pass=1)
    assert n2 == n - 70 and "page 02.png" not in [c[0] for c in store2.calls] and emb2.passes == [65, 70, 133, 8]
    # one wave for everything when the threshold is large; a byte cap closes waves too
    n3, emb3, _ = run(wave=10_000)
    assert n3 == n and emb3.passes == [276]
    assert engine_threads == {threading.get_ident()}  # crop_boxes and the passes ran on the calling thread, never the producer's
