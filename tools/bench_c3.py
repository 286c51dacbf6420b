#!/usr/bin/env python3
"""Config C3: 4096 variable-size crops (the size distribution of the reference's 1862 bundled
region crops, cycled; pixels synthetic because the crops themselves cannot travel) through the
on-GPU resize / normalise / patchify (K1) and the embedder.  Prints K1 time, algorithmic bytes,
GB/s and whole-path crops/s, and checks a sample against the oracle bit-for-bit (patches).

`--resize-rule fit_pad|clip` runs all of that under one rule of mme_set_resize_rule (default fit_pad).  `--resize-rule both`
alternates K1 under the two rules in one process on the same crops -- two warm-ups each, then five timed runs of each,
interleaved, one line per run -- and then times one mme_embed step of seeded CLIP-B/16 under each rule.  `--resize-rule specs`
does the same over the two rules and the four specs of mme_set_resize_spec that real checkpoints ask for (SPECS below).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multimodal_embeddings_amd._lib import Engine, ResizeSpec
from multimodal_embeddings_amd.weights import make_vit_weights, round_to_bf16


def k1_ms(eng, pix, offs, hw):
    """kernel time of one mme_preprocess call (the context's event pairs)"""
    eng.profile(True)
    eng.preprocess(pix, offs, hw)
    torch.cuda.synchronize()
    return eng.profile_read()["preprocess"][0]


SPECS = {  # the rules real checkpoints ask for (tests/resize_spec_reference.py)
    "exact224_bicubic": ResizeSpec("exact", 224, 224, 3),
    "exact224_bilinear": ResizeSpec("exact", 224, 224, 2),
    "edge256_bicubic": ResizeSpec("shortest_edge", 256, 0, 3),
    "exact256_bicubic": ResizeSpec("exact", 256, 256, 3),
}


def set_rule(eng, rule):
    if rule in SPECS:
        eng.set_resize_spec(SPECS[rule])
    else:
        eng.set_resize_rule(rule)


def both_rules(pix, offs, hw, n, rules=("fit_pad", "clip")):
    from multimodal_embeddings_amd.weights import make_clip_weights

    eng = Engine(0)
    eng.load_clip(make_clip_weights(1))
    for _ in range(2):
        for rule in rules:
            set_rule(eng, rule)
            k1_ms(eng, pix, offs, hw)
    ms = {r: [] for r in rules}
    for i in range(5):
        for rule in rules:
            set_rule(eng, rule)
            ms[rule].append(k1_ms(eng, pix, offs, hw))
            print(f"C3 K1 run {i} rule {rule}: kernels {ms[rule][-1]:.3f} ms")
    eng.profile(False)
    for rule in rules:
        v = ms[rule]
        print(f"C3 K1 rule {rule}: min {min(v):.3f} median {sorted(v)[2]:.3f} max {max(v):.3f} ms over 5 runs")
    for rule in rules[1:]:
        print(f"C3 K1 ratio {rule} / fit_pad (medians): {sorted(ms[rule])[2] / sorted(ms['fit_pad'])[2]:.2f}")
    for rule in rules:
        set_rule(eng, rule)
        for _ in range(2):
            eng.embed(pix, offs, hw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.embed(pix, offs, hw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"C3 embed CLIP-B/16 rule {rule}: {dt*1e3:.1f} ms for {n} crops ({n / dt:.0f} crops/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resize-rule", choices=("fit_pad", "clip", "both", "specs"), default="fit_pad")
    rule = ap.parse_args().resize_rule
    n = 4096
    sizes = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "bundled_crop_sizes_hw.npy"))
    hw = sizes[np.arange(n) % len(sizes)].astype(np.int32)
    nbytes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum((nbytes[:-1] + 15) // 16 * 16)
    total = int(offs[-1] + nbytes[-1]) + 16
    g = torch.Generator(device="cuda").manual_seed(0)
    pix = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
    if rule == "both":
        return both_rules(pix, offs, hw, n)
    if rule == "specs":
        return both_rules(pix, offs, hw, n, ("fit_pad", "clip") + tuple(SPECS))
    eng = Engine(0)
    eng.load_vit(make_vit_weights(seed=1))
    eng.set_resize_rule(rule)
    eng.profile(True)
    for _ in range(2):
        patches = eng.preprocess(pix, offs, hw)
    torch.cuda.synchronize()
    eng.profile(True)
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        patches = eng.preprocess(pix, offs, hw)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    prof = eng.profile_read()
    k1_ms = prof["preprocess"][0] / reps
    alg = float(nbytes.sum()) + n * 301056.0
    print(f"C3 K1: {n} crops, {nbytes.sum()/1e6:.1f} MB of pixels, algorithmic {alg/1e9:.3f} GB; kernels {k1_ms:.3f} ms "
          f"({alg/k1_ms/1e6:.0f} GB/s), wall incl. host crop table + H2D {wall*1e3:.2f} ms")
    # whole path
    for _ in range(2):
        eng.embed(pix, offs, hw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        e32, _ = eng.embed(pix, offs, hw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    print(f"C3 embed: {n / dt:.0f} crops/s ({dt*1e3:.1f} ms)")
    # sample parity (bit-exact patches)
    from oracle import preprocess as opre

    host = pix.cpu().numpy()
    got = patches.float().cpu().numpy().reshape(n, 196, 768)
    for i in (0, 1, 17, 500, 1861, 4095):
        h, w = hw[i]
        a = host[offs[i] : offs[i] + nbytes[i]].reshape(h, w, 3)
        if rule == "clip":
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
            from clip_preprocess_reference import clip_window_u8

            lut = opre.normalise_lut()
            win = clip_window_u8(a)
            want = opre.patchify(np.stack([lut[ch][win[:, :, ch]] for ch in range(3)]))
        else:
            want = opre.preprocess_to_patches(a)
        assert np.array_equal(got[i], round_to_bf16(want)), i
    print("C3 sample parity: bit-exact")


if __name__ == "__main__":
    main()
