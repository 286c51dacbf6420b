"""Writes tests/golden/mllama_lm_cases.npz: inputs and `hidden_states[-1]` of transformers' MllamaForConditionalGeneration (fp32,
on the CPU) on the seeded towers of tests/mllama_lm_reference.py (GOLDEN_TOWERS).  No weights are recorded: the language model
and the projector are `weights.make_mllama_lm_weights`, and the tiny vision model (whose weights are torch's seeded
initialisation) only produces the recorded vision states.

    python tests/golden/make_mllama_lm_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mllama_lm_reference as R  # noqa: E402
from transformers import MllamaConfig, MllamaForConditionalGeneration  # noqa: E402
from transformers.models.mllama.configuration_mllama import MllamaTextConfig, MllamaVisionConfig  # noqa: E402

BOS, IMG, PAD = 1, 300, 299
ASPECT_ID = {1: 1, 2: 2, 4: 6}  # (1, 1), (1, 2), (2, 2) among the canvases of at most four tiles


def build(name):
    w, g = R.golden_tower(name)
    v = MllamaVisionConfig(hidden_size=32, attention_heads=2, intermediate_size=64, num_hidden_layers=1, num_global_layers=1, image_size=28, patch_size=14,
                           max_num_tiles=4, intermediate_layers_indices=[0], vision_output_dim=g.vision_output_dim)
    t = MllamaTextConfig(vocab_size=g.vocab_size, hidden_size=g.hidden_size, num_attention_heads=g.num_heads, num_key_value_heads=g.num_kv_heads,
                         intermediate_size=g.intermediate_size, num_hidden_layers=g.num_layers, cross_attention_layers=list(g.cross_attention_layers),
                         rms_norm_eps=g.rms_norm_eps, max_position_embeddings=512, hidden_act=g.hidden_act,
                         rope_parameters={"rope_type": g.rope_type, "rope_theta": g.rope_theta, "factor": g.rope_factor, "low_freq_factor": g.rope_low_freq_factor,
                                          "high_freq_factor": g.rope_high_freq_factor, "original_max_position_embeddings": g.rope_original_max},
                         pad_token_id=PAD, bos_token_id=BOS, eos_token_id=2)
    torch.manual_seed(0)
    m = MllamaForConditionalGeneration(MllamaConfig(vision_config=v, text_config=t, image_token_index=g.image_token_id)).eval().float()
    sd = m.state_dict()
    for k, a in w.items():
        key = "model." + k
        assert tuple(sd[key].shape) == tuple(a.shape), (key, sd[key].shape, a.shape)
        sd[key] = torch.from_numpy(np.ascontiguousarray(a))
    m.load_state_dict(sd)
    inv = m.model.language_model.rotary_emb.inv_freq.numpy()
    return m, g, inv


def image_case(m, g, ids, lengths, tiles, seed):
    ids = np.asarray(ids, dtype=np.int64)
    n, S = ids.shape
    gen = torch.Generator().manual_seed(seed)
    pv = torch.randn(n, 1, 4, 3, 28, 28, generator=gen)
    ar_ids = torch.tensor([[ASPECT_ID[t]] for t in tiles])
    ar_mask = torch.zeros(n, 1, 4, dtype=torch.long)
    am = torch.zeros(n, S, dtype=torch.long)
    cam = torch.zeros(n, S, 1, 4)
    xmask = np.zeros((n, S), dtype=np.uint8)
    for b in range(n):
        ar_mask[b, 0, : tiles[b]] = 1
        pv[b, 0, tiles[b]:] = 0  # padding tiles are zero pixels, as the processor leaves them
        am[b, : lengths[b]] = 1
        first = int(np.argmax(ids[b] == g.image_token_id))
        cam[b, first:, 0, : tiles[b]] = 1
        xmask[b, first:] = (1 << tiles[b]) - 1
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(ids), attention_mask=am, pixel_values=pv, aspect_ratio_ids=ar_ids, aspect_ratio_mask=ar_mask,
                cross_attention_mask=cam, return_dict=True, output_hidden_states=True)
        vo = m.model.vision_model(pixel_values=pv, aspect_ratio_ids=ar_ids, aspect_ratio_mask=ar_mask).last_hidden_state
    return {"ids": ids.astype(np.int32), "lengths": np.asarray(lengths, dtype=np.int32), "num_tiles": np.asarray(tiles, dtype=np.int32), "xmask": xmask,
            "vision": vo[:, 0].numpy().astype(np.float32), "hidden": out.hidden_states[-1].numpy().astype(np.float32)}


def text_case(m, ids, lengths):
    ids = np.asarray(ids, dtype=np.int64)
    n, S = ids.shape
    am = torch.zeros(n, S, dtype=torch.long)
    for b in range(n):
        am[b, : lengths[b]] = 1
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(ids), attention_mask=am, return_dict=True, output_hidden_states=True)
    return {"ids": ids.astype(np.int32), "lengths": np.asarray(lengths, dtype=np.int32), "hidden": out.hidden_states[-1].numpy().astype(np.float32)}


def padded(rows, S):
    return [r + [PAD] * (S - len(r)) for r in rows]


def main():
    rng = np.random.default_rng(11)
    words = lambda k: [int(x) for x in rng.integers(3, 290, size=k)]  # noqa: E731
    out = {}
    m, g, inv = build("a")
    out["a.inv_freq"] = inv.astype(np.float32)
    tail = words(5)
    cases = {
        "bos_first": image_case(m, g, [[BOS, IMG, BOS] + tail] * 3, [8, 8, 8], [1, 2, 4], 1),      # row 0 attends no tile
        "image_first": image_case(m, g, [[IMG, BOS] + tail] * 3, [7, 7, 7], [1, 2, 4], 2),
        "two_lengths": image_case(m, g, padded([[BOS, IMG, BOS] + words(9), [BOS, IMG, BOS] + words(3)], 12), [12, 6], [2, 4], 3),
        "text_only": text_case(m, padded([[BOS] + words(4), [BOS] + words(39)], 40), [5, 40]),
    }
    m, g, inv = build("b")
    out["b.inv_freq"] = inv.astype(np.float32)
    cases["cross_0_2"] = image_case(m, g, padded([[BOS, IMG, BOS] + words(6), [IMG, BOS] + words(4)], 9), [9, 6], [2, 1], 4)
    for name, fields in cases.items():
        for k, v in fields.items():
            out[f"{name}.{k}"] = v
    path = os.path.join(HERE, "mllama_lm_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
