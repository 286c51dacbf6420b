"""float64 numpy restatement of the Mllama language tower, independent of transformers: projector,
MllamaTextModel's self- and cross-attention layers, the cross-attention mask, the final norm and last-token pooling.

`forward(w, geom, ids, lengths, vision, xmask, mutant=None)` returns the rows AFTER the final RMSNorm, [n, S, hidden]
(`hidden_states[-1]` of transformers); `pooled(...)` the L2-normalised row at len - 1.  `mutant` names ONE deliberate
mistake (MUTANTS), for the sharpness tests: each is a tower somebody could plausibly have written instead.

The per-kernel functions (rmsnorm, headnorm, rope, silu_mul, self_attention, cross_attention) are what the GPU tests
compare single launches against.
"""
from __future__ import annotations

import numpy as np

from multimodal_embeddings_amd import weights as W

MUTANTS = ("no_rope", "interleaved_rope", "default_rope", "no_q_norm", "no_k_norm", "k_norm_on_v", "cross_in_text_only", "no_causal_mask",
           "kv_head_modulo", "padding_tiles_attended", "masked_row_attends_nothing", "masked_row_mlp_kept", "raw_gate", "pre_norm_pooled",
           "last_row_pooled", "no_projector_bias")


def rmsnorm(x, w, eps):
    x = np.asarray(x, dtype=np.float64)
    return np.asarray(w, dtype=np.float64) * (x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps))


def headnorm(x, w, eps):
    """x [..., heads * 128]: every head of 128 normalised with w [128]"""
    x = np.asarray(x, dtype=np.float64)
    h = x.reshape(x.shape[:-1] + (-1, 128))
    return rmsnorm(h, w, eps).reshape(x.shape)


def rope(x, cos, sin, interleaved=False):
    """x [S, heads, 128], cos / sin [S, 64]: the rotate_half form (pairs (d, d + 64)); interleaved: pairs (2 d, 2 d + 1)"""
    x = np.asarray(x, dtype=np.float64)
    c, s = np.asarray(cos, dtype=np.float64)[:, None, :], np.asarray(sin, dtype=np.float64)[:, None, :]
    out = np.empty_like(x)
    if interleaved:
        a, b = x[..., 0::2], x[..., 1::2]
        out[..., 0::2], out[..., 1::2] = a * c - b * s, b * c + a * s
    else:
        a, b = x[..., :64], x[..., 64:]
        out[..., :64], out[..., 64:] = a * c - b * s, b * c + a * s
    return out


def silu_mul(g, u):
    g = np.asarray(g, dtype=np.float64)
    return g / (1.0 + np.exp(-g)) * np.asarray(u, dtype=np.float64)


def softmax(s):
    s = s - np.max(s, axis=-1, keepdims=True)
    e = np.exp(s)
    return e / np.sum(e, axis=-1, keepdims=True)


def self_attention(q, k, v, causal=True, kv_of=None):
    """q [S, H, 128], k / v [S, KVH, 128] -> [S, H, 128]; head h reads KV head h // (H / KVH) (kv_of overrides)"""
    S, H, _ = q.shape
    KVH = k.shape[1]
    out = np.empty((S, H, 128))
    mask = np.triu(np.ones((S, S), dtype=bool), 1)
    for h in range(H):
        j = kv_of(h) if kv_of else h // (H // KVH)
        s = q[:, h] @ k[:, j].T * 128 ** -0.5
        if causal:
            s = np.where(mask, -np.inf, s)
        out[:, h] = softmax(s) @ v[:, j]
    return out


def cross_attention(q, k, v, bits, tokens, unmask_empty=True, kv_of=None):
    """q [S, H, 128], k / v [tiles * tokens, KVH, 128], bits [S] (the tiles a row attends) -> [S, H, 128].  A row with no bit
    attends every key (transformers multiplies its additive mask to zero); unmask_empty False leaves it a zero row."""
    S, H, _ = q.shape
    KVH = k.shape[1]
    tile_of = np.arange(k.shape[0]) // tokens
    bits = np.asarray(bits).astype(np.int64)
    allowed = ((bits[:, None] >> tile_of[None, :]) & 1).astype(bool)
    empty = bits == 0
    if unmask_empty:
        allowed[empty] = True
    out = np.zeros((S, H, 128))
    for h in range(H):
        j = kv_of(h) if kv_of else h // (H // KVH)
        s = np.where(allowed, q[:, h] @ k[:, j].T * 128 ** -0.5, -np.inf)
        rows = allowed.any(axis=1)
        out[rows, h] = softmax(s[rows]) @ v[:, j]
    return out


def processor_mask(ids, num_tiles, image_token_id):
    """The processor's rule as bits [n, S]: rows from the first image token on attend tiles [0, num_tiles), rows before it none."""
    ids = np.asarray(ids)
    out = np.zeros(ids.shape, dtype=np.uint8)
    for b in range(ids.shape[0]):
        first = int(np.argmax(ids[b] == image_token_id))
        out[b, first:] = (1 << int(num_tiles[b])) - 1
    return out


def forward(w, geom, ids, lengths=None, vision=None, xmask=None, mutant=None):
    """ids [n, S]; vision [n, tiles, tokens, F] or None; xmask uint8 [n, S] -> float64 [n, S, hidden] after the final norm.
    The padded positions (at or behind lengths[b]) are computed like any other: under the causal mask they reach no row before them."""
    assert mutant is None or mutant in MUTANTS, mutant
    f64 = lambda name: np.asarray(w[name], dtype=np.float64)  # noqa: E731
    ids = np.asarray(ids)
    n, S = ids.shape
    D, H, KVH, eps = geom.hidden_size, geom.num_heads, geom.num_kv_heads, geom.rms_norm_eps
    import dataclasses

    rope_geom = dataclasses.replace(geom, rope_type="default") if mutant == "default_rope" else geom
    inv = W.mllama_rope_inv_freq(rope_geom).astype(np.float64)
    ang = np.arange(S, dtype=np.float64)[:, None] * inv[None, :]
    cos, sin = np.cos(ang), np.sin(ang)
    kv_of = (lambda h: h % KVH) if mutant == "kv_head_modulo" else None
    gate = (lambda g: g) if mutant == "raw_gate" else np.tanh
    cross = set(geom.cross_layers)
    out = np.empty((n, S, D))
    for b in range(n):
        x = f64("language_model.embed_tokens.weight")[ids[b]]
        vis = None
        if vision is not None:
            st = np.asarray(vision[b], dtype=np.float64)
            tiles, tokens, F = st.shape
            vis = st.reshape(tiles * tokens, F) @ f64("multi_modal_projector.weight").T
            if mutant != "no_projector_bias":
                vis = vis + f64("multi_modal_projector.bias")
            bits = np.asarray(xmask[b]).astype(np.int64)
            if mutant == "padding_tiles_attended":
                bits = np.where(bits != 0, (1 << tiles) - 1, 0)
        elif mutant == "cross_in_text_only":  # a tower that runs the cross layers over an all-zero image instead of skipping them
            tiles, tokens = 1, 1
            vis = np.zeros((1, D)) + f64("multi_modal_projector.bias")
            bits = np.ones(S, dtype=np.int64)
        for l in range(geom.num_layers):
            p = f"language_model.layers.{l}."
            if l in cross:
                if vis is None:
                    continue
                a = p + "cross_attn."
                hn = rmsnorm(x, f64(p + "input_layernorm.weight"), eps)
                q = hn @ f64(a + "q_proj.weight").T
                k = vis @ f64(a + "k_proj.weight").T
                v = vis @ f64(a + "v_proj.weight").T
                if mutant != "no_q_norm":
                    q = headnorm(q, f64(a + "q_norm.weight"), eps)
                if mutant not in ("no_k_norm", "k_norm_on_v"):
                    k = headnorm(k, f64(a + "k_norm.weight"), eps)
                if mutant == "k_norm_on_v":
                    v = headnorm(v, f64(a + "k_norm.weight"), eps)
                att = cross_attention(q.reshape(S, H, 128), k.reshape(-1, KVH, 128), v.reshape(-1, KVH, 128), bits, tokens,
                                      unmask_empty=mutant != "masked_row_attends_nothing", kv_of=kv_of)
                x = x + gate(float(f64(p + "cross_attn_attn_gate").reshape(-1)[0])) * (att.reshape(S, D) @ f64(a + "o_proj.weight").T)
                row_mask = np.ones(S) if mutant == "masked_row_mlp_kept" else (bits != 0).astype(np.float64)
                hn = rmsnorm(x, f64(p + "post_attention_layernorm.weight"), eps)
                mlp = silu_mul(hn @ f64(p + "mlp.gate_proj.weight").T, hn @ f64(p + "mlp.up_proj.weight").T) @ f64(p + "mlp.down_proj.weight").T
                x = x + gate(float(f64(p + "cross_attn_mlp_gate").reshape(-1)[0])) * row_mask[:, None] * mlp
            else:
                a = p + "self_attn."
                hn = rmsnorm(x, f64(p + "input_layernorm.weight"), eps)
                q = (hn @ f64(a + "q_proj.weight").T).reshape(S, H, 128)
                k = (hn @ f64(a + "k_proj.weight").T).reshape(S, KVH, 128)
                v = (hn @ f64(a + "v_proj.weight").T).reshape(S, KVH, 128)
                if mutant != "no_rope":
                    q, k = (rope(t, cos, sin, interleaved=mutant == "interleaved_rope") for t in (q, k))
                att = self_attention(q, k, v, causal=mutant != "no_causal_mask", kv_of=kv_of)
                x = x + att.reshape(S, D) @ f64(a + "o_proj.weight").T
                hn = rmsnorm(x, f64(p + "post_attention_layernorm.weight"), eps)
                x = x + silu_mul(hn @ f64(p + "mlp.gate_proj.weight").T, hn @ f64(p + "mlp.up_proj.weight").T) @ f64(p + "mlp.down_proj.weight").T
        out[b] = x if mutant == "pre_norm_pooled" else rmsnorm(x, f64("language_model.norm.weight"), eps)
    return out


def pooled(w, geom, ids, lengths=None, vision=None, xmask=None, mutant=None):
    """The embedding: the row at lengths[b] - 1 of forward(), divided by max(its L2 norm, 1e-12) -> [n, hidden]"""
    ids = np.asarray(ids)
    n, S = ids.shape
    lengths = np.full(n, S) if lengths is None else np.asarray(lengths)
    hs = forward(w, geom, ids, lengths, vision, xmask, mutant)
    rows = np.stack([hs[b, (S if mutant == "last_row_pooled" else int(lengths[b])) - 1] for b in range(n)])
    return rows / np.maximum(np.linalg.norm(rows, axis=-1, keepdims=True), 1e-12)


# ---- the towers of tests/golden/mllama_lm_cases.npz (tests/golden/make_mllama_lm_golden.py) ------------------------------
# llama3 frequencies with original_max_position_embeddings 32: of the 64 frequencies some keep their value, some are divided
# by 8 and some are interpolated, so a tower with the `default` rule differs in every band.
GOLDEN_BASE = W.MllamaLMGeometry(hidden_size=512, num_heads=4, num_kv_heads=2, intermediate_size=1024, num_layers=3, cross_attention_layers=(1,),
                                 vocab_size=300, vision_output_dim=64, image_token_id=300, rope_original_max=32)
GOLDEN_TOWERS = {
    "a": (7, GOLDEN_BASE),
    "b": (8, W.MllamaLMGeometry(hidden_size=512, num_heads=4, num_kv_heads=4, intermediate_size=1024, num_layers=3, cross_attention_layers=(0, 2),
                               vocab_size=300, vision_output_dim=64, image_token_id=300, rope_original_max=32)),
}
GOLDEN_TOKENS = 5  # tokens per tile of the golden vision model (28 x 28 tiles, patch 14, + the class token)
# case -> (tower, fields); every case holds ids [n, S], lengths [n], hidden f32 [n, S, 512]; image cases also vision f32
# [n, 4, 5, 64], num_tiles [n], xmask uint8 [n, S]
GOLDEN_CASES = {"bos_first": "a", "image_first": "a", "two_lengths": "a", "text_only": "a", "cross_0_2": "b"}


def golden_tower(name):
    seed, geom = GOLDEN_TOWERS[name]
    return W.make_mllama_lm_weights(seed, geom), geom
