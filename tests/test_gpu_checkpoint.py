"""Checkpoint directory -> device-side weight preparation (csrc/weight_prep.hip) -> embeddings.

Each encoder's load is one sequence of buffers (csrc/weight_load.hip, csrc/capi_tilevit.hip) run by two preparers: the host
loops behind mme_load_vit / mme_load_tile_vit and the kernels behind mme_load_*_as, operation for operation.  So everything
here is EQUALITY between the two preparers: the fingerprints of the prepared buffers (mme_weights_fingerprint) agree word
for word with a context loaded by the host path from the same values, and the embeddings are bit-equal.  Neither preparer
is the reference of the other's arithmetic -- they share one sequence: tests/test_gpu_weight_prep.py compares every prepared
buffer, and the fingerprint itself, with float64 from the model's definition.  Seed 7: `model_name` used to be ignored, so a
directory of seed-7 weights only gives seed-7 vectors when it is really read."""
import json

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd import checkpoint as ckpt
from multimodal_embeddings_amd._lib import Engine
from multimodal_embeddings_amd.embedder import RegionEmbedder
from multimodal_embeddings_amd.weights import TileViTGeometry, make_tile_vit_weights, make_vit_weights, synthetic_crops

pytestmark = pytest.mark.gpu

SEED = 7
SHALLOW = TileViTGeometry(num_layers=2, num_global_layers=1, intermediate_layers=(0,))
VIT_BUFFERS = 6 + 12 * 18   # mme_load_vit: six tables, then 18 buffers per layer
TILE_BUFFERS = 11 + 3 * 9   # mme_load_tile_vit at the shallow geometry: eleven tables, then 9 buffers per layer


@pytest.fixture(scope="module")
def vit_w():
    return make_vit_weights(SEED)


@pytest.fixture(scope="module")
def crops():
    return torch.from_numpy(synthetic_crops(64, seed=3)).cuda()


def _close(embedder):
    for e in embedder.engines:
        e.close()


def _embed(embedder, crops):
    e32, e16 = embedder.embed_uniform(crops)
    torch.cuda.synchronize()
    return e32.cpu().numpy().view(np.uint32), e16.cpu().view(torch.int16).numpy()


@pytest.fixture(scope="module")
def default_seed_embeddings(crops):
    emb = RegionEmbedder(device=0, chunk=64)
    out = _embed(emb, crops)
    _close(emb)
    return out


def _host_dict(ck):
    """The checkpoint's tensors widened to f32 on the host: what the host path (Engine.load_vit) is given."""
    return {k: t.float().numpy() for k, t in ck.tensors.items()}


def _assert_same_fingerprint(got, want, count):
    assert len(got) == len(want) == count, (len(got), len(want), count)
    differ = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, f"prepared buffers {differ[:20]} (of {count}, in creation order) differ between the device and the host path"


def _vit_fingerprints(ck):
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_vit_checkpoint(ck)
        host.load_vit(_host_dict(ck), eps=ck.geometry.layer_norm_eps)
        return dev.weights_fingerprint(), host.weights_fingerprint()
    finally:
        dev.close()
        host.close()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_vit_directory_matches_host_path(tmp_path, vit_w, crops, default_seed_embeddings, dtype):
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", dtype)
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    assert ck.dtype == dtype
    got, want = _vit_fingerprints(ck)
    print(f"{dtype}: {sum(a == b for a, b in zip(got, want))} of {len(want)} fingerprint words equal")
    _assert_same_fingerprint(got, want, VIT_BUFFERS)
    assert len(set(want)) > VIT_BUFFERS // 2  # the checksum tells buffers apart

    from_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, allow_synthetic=False)
    assert from_dir.checkpoint is not None and from_dir.checkpoint.dtype == dtype
    from_dict = RegionEmbedder(weights=_host_dict(ck), device=0, chunk=64)
    try:
        a32, a16 = _embed(from_dir, crops)
        b32, b16 = _embed(from_dict, crops)
    finally:
        _close(from_dir)
        _close(from_dict)
    print(f"{dtype}: f32 rows differing {int((a32 != b32).any(axis=1).sum())}, bf16 rows differing {int((a16 != b16).any(axis=1).sum())} of 64")
    assert np.array_equal(a32, b32) and np.array_equal(a16, b16)
    d32, d16 = default_seed_embeddings
    assert not np.array_equal(a32, d32) and not np.array_equal(a16, d16)


def test_planted_values_fingerprints(tmp_path, vit_w):
    """-0.0, an f32 subnormal, a bf16 rounding tie and a value near f32's top, planted where the fold multiplies, rounds and
    sums them: no flushing, the same ties, the same f64 sums as the host loop."""
    w = {k: v.copy() for k, v in vit_w.items()}
    planted = np.array([-0.0, 1e-39, 1.0 + 2.0 ** -8, 1e38], dtype=np.float32)
    g, b = w["layers.0.layernorm_before.weight"], w["layers.0.layernorm_before.bias"]
    g[5] = 1.0        # w * gamma = w at column 5: the tie reaches the bf16 rounding as it is
    b[9] = 1e-39      # a subnormal beta
    g2, b2 = w["layers.0.layernorm_after.weight"], w["layers.0.layernorm_after.bias"]
    g2[5] = 1.0 + 2.0 ** -8
    b2[9] = -0.0
    for name in ("layers.0.attention.q_proj.weight", "layers.0.mlp.fc1.weight"):
        m = w[name]
        for r, row in enumerate((0, 63, 64, 767)):
            m[row, 5] = planted[r]
            m[row, 9] = planted[(r + 1) % 4]
            m[row, 700 + r] = planted[(r + 2) % 4]
    w["layers.0.attention.q_proj.bias"][:4] = planted
    w["layers.0.mlp.fc1.bias"][:4] = planted
    w["layers.0.attention.o_proj.weight"][3, :4] = planted  # the plain conversion
    w["embeddings.position_embeddings"].reshape(-1)[:4] = planted  # an f32 table
    ckpt.save_checkpoint(tmp_path, w, "vit_b16", "float32")
    ck = ckpt.read_checkpoint(tmp_path, "vit_b16")
    assert ck.tensors["layers.0.mlp.fc1.weight"][63, 5].item() == float(np.float32(1e-39)) != 0.0
    got, want = _vit_fingerprints(ck)
    _assert_same_fingerprint(got, want, VIT_BUFFERS)
    # and the planted values do reach the prepared buffers: the unplanted checkpoint's fingerprint is another one
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "float32")
    plain, _ = _vit_fingerprints(ckpt.read_checkpoint(tmp_path, "vit_b16"))
    assert plain != got and plain[-1] == got[-1]  # layer 11's last buffer is untouched


def test_tile_tower_directory_matches_host_path(tmp_path):
    w = make_tile_vit_weights(SEED, SHALLOW)
    ckpt.save_checkpoint(tmp_path, w, "mllama_tiles", "bfloat16", SHALLOW)
    ck = ckpt.read_checkpoint(tmp_path, "mllama_tiles")
    assert ck.dtype == "bfloat16" and ck.geometry == SHALLOW
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_tile_vit_checkpoint(ck)
        host.load_tile_vit(w, SHALLOW)
        got, want = dev.weights_fingerprint(), host.weights_fingerprint()
    finally:
        dev.close()
        host.close()
    _assert_same_fingerprint(got, want, TILE_BUFFERS)

    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(560, 560, 3), (300, 900, 3), (1200, 500, 3), (700, 800, 3)]]
    from_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64, encoder="mllama_tiles", allow_synthetic=False)
    from_dict = RegionEmbedder(weights=w, geometry=SHALLOW, device=0, chunk=64, encoder="mllama_tiles")
    try:
        a, ok_a = from_dir.get_image_embeddings(images, as_array=True)
        b, ok_b = from_dict.get_image_embeddings(images, as_array=True)
    finally:
        _close(from_dir)
        _close(from_dict)
    assert ok_a.all() and ok_b.all() and a.shape == (4, SHALLOW.output_dim)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(a).max() > 0


def test_preprocessor_mean_std_are_applied(tmp_path, vit_w, crops):
    half = (0.5, 0.5, 0.5)
    ckpt.save_checkpoint(tmp_path, vit_w, "vit_b16", "bfloat16", image_mean=half, image_std=half)
    assert json.loads((tmp_path / "preprocessor_config.json").read_text())["image_mean"] == [0.5, 0.5, 0.5]
    from_dir = RegionEmbedder(str(tmp_path), device=0, chunk=64)
    by_hand = RegionEmbedder(weights=vit_w, device=0, chunk=64)
    clip = RegionEmbedder(weights=vit_w, device=0, chunk=64)
    try:
        for e in by_hand.engines:
            e.set_normalisation(half, half)
        a32, a16 = _embed(from_dir, crops)
        b32, b16 = _embed(by_hand, crops)
        c32, _ = _embed(clip, crops)
    finally:
        for emb in (from_dir, by_hand, clip):
            _close(emb)
    assert from_dir.checkpoint.image_mean == half
    assert np.array_equal(a32, b32) and np.array_equal(a16, b16)
    assert not np.array_equal(a32, c32)  # and the constants matter: the default (CLIP) normalisation gives other vectors
