#!/usr/bin/env python3
"""sha256 of what every encoder pass writes, per configuration: one JSON line each.

    python tools/pass_hashes.py [--only image|text|tile|rows|resample] > hashes.jsonl

For a change that moves no arithmetic (the transformer block's launch sequence is host code: csrc/encoder_pass.hip; the
row kernels share their device-side pieces: csrc/row_kernels.h; the three resize paths share Pillow's 8-bit resampling:
csrc/resample.h) the lines of two libraries must be EQUAL, not close.  Run the tool once per library, each in a fresh process -- another
build is selected with MME_LIB_PATH and MME_ALLOW_LIB_OVERRIDE=1, as tools/_diag.py does -- and compare the outputs with
`diff`.  Every tower is two layers deep and seeded (weights.py), every input is seeded; the shapes are the smallest that
reach every branch of the shared block:

  image   ViT-S/16 width (384: no partial planes under ln_mode 2), ViT-B/16 width (768: planes), CLIP-B/16 (pre-LN,
          QuickGELU, projection), ViT-B/32, CLIP-B/32, SigLIP-B/16 (196 tokens, tanh-GELU, pooling head), DINOv2-B/14
          (257 tokens).  3 crops at patch 16 are 591 rows (two 256-row panels and a ragged tail of 79), 6 crops at patch
          32 are 300, 3 crops at patch 14 are 771 (three panels and a ragged 3).  From the defaults one switch at a time:
          ln_mode, tile order, attention mode, last-layer pruning at the first and the last pool token, GEMM variant, and
          chunks of 2 over 5 crops.  The token rows (`vit_tokens`) at the defaults, with pruning on (the token pass runs
          the last block unpruned) and in chunks of 2 over 5 crops (three chunks, the last ragged: the token pointer's
          offset per chunk).  The pixel path (`embed`, `embed_tokens`) in chunks of 2 over 5 crops for one tower per
          retile form: vit_b16 (none), vit_b32, dinov2_b14.
  text    CLIP-B's text width with and without projection, 3 sequences; once more than one chunk of 1024.  The SigLIP
          text tower (64 tokens, head with bias) on 3 sequences.
  tile    1 local + 1 global layer, one intermediate state, both save-point conventions, ln_mode 1 / 2 x attention mode
          0 / 1 / 2, on a 1-tile and a 4-tile image.
  rows    every row launcher once through the *_apply hooks, at every width it is built for: LayerNorm, statistics,
          class rows, pooled LayerNorm with and without the L2 step at the first and the last token of the 197- and the
          50-token layout and with it of the 257-token layout, pre-LN, the embed rows of the 196-token layout (no class
          token) and of the 50- and the 257-token layout (2 crops: the class row of the second is reached), the EOS pooling of both text layouts, the three L2 forms at p = 64 / 320 /
          1024 (one partly filled column group, a partly filled second one, all four).  5 rows or sequences: two
          workgroups of four waves, the second with one live wave.  Every output buffer is hashed WITH a sentinel-filled
          margin behind it, untouched rows included.
  resample  every resize path, each run ONE call on a small mixed batch in one fixed seeded order: `preprocess` under the
          fit_pad and the clip rule, each with a normalisation the patch emitter computes (fma) and one it reads from the
          table; `preprocess_tiles` (560, 4); `lanczos_resize` in the ordinary and in the vertical-first order (more than
          100 times as high as wide, getting lower).  The batch: 1 x 1, 20 x 63, 63 x 20, crops that keep their width or
          their height (300 x 224, 224 x 300, 100 x 224) and, per rule, the shapes whose horizontal pass is of class 1
          and of class 2 (fit_pad 1400 x 1350 and 17 x 8000, clip 37 x 1000 and 2000 x 3000); 224 x 224 alone runs the
          RESIZE = false instantiation.  Every output buffer is hashed with its sentinel margin.

Each configuration ends in a device synchronise; the first error ends the run (nothing is caught).  Needs a GPU.
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("image", "text", "tile", "rows", "resample"), default=None)
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from multimodal_embeddings_amd import weights as W
    from multimodal_embeddings_amd._lib import Engine

    if not torch.cuda.is_available():
        raise SystemExit("pass_hashes: no GPU visible; the passes run on the GPU and there is no fallback")

    def pack(arrays):
        """list of uint8 [h, w, 3] -> (pix CUDA tensor, offs int64 [n], hw int32 [n, 2]), every crop 16-byte aligned"""
        hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
        sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
        offs = np.zeros(len(arrays), dtype=np.int64)
        offs[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
        buf = np.zeros(int(offs[-1] + sizes[-1]) + 16, dtype=np.uint8)
        for a, o, n in zip(arrays, offs, sizes):
            buf[o : o + n] = a.reshape(-1)
        return torch.from_numpy(buf).to("cuda:0"), offs, hw

    def emit(config: str, *tensors):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        print(json.dumps({"config": config, "sha256": h.hexdigest()}), flush=True)

    def image():
        two = {"num_layers": 2}
        towers = {
            "vit_s16": dataclasses.replace(W.VIT_S16, **two), "vit_b16": dataclasses.replace(W.VIT_B16, **two),
            "clip_b16": dataclasses.replace(W.CLIP_B16, **two), "vit_b32": dataclasses.replace(W.VIT_B32, **two),
            "clip_b32": dataclasses.replace(W.CLIP_B32, **two), "siglip_b16": dataclasses.replace(W.SIGLIP_B16, **two),
            "dinov2_b14": dataclasses.replace(W.DINOV2_B14, **two),
        }
        # (name, setter, values): the first value is the library's default and is restored after the sweep
        switches = [("ln_mode", Engine.set_ln_fusion, (2, 0, 1)), ("tile_order", Engine.set_tile_order, (1, 0, 2)),
                    ("attention_mode", Engine.set_attention_mode, (1, 0, 2)), ("gemm_variant", Engine.set_gemm_variant, (0, 1, 3))]
        for name, geom in towers.items():
            e = Engine(0)
            if isinstance(geom, W.SiglipGeometry):
                e.load_siglip(W.make_siglip_weights(11, geom), geom=geom)
            elif isinstance(geom, W.Dinov2Geometry):
                e.load_dinov2(W.make_dinov2_weights(11, geom), geom=geom)
            elif isinstance(geom, W.CLIPGeometry):
                e.load_clip(W.make_clip_weights(11, geom), geom=geom)
            else:
                e.load_vit(W.make_vit_weights(11, geom), geom=geom)
            n = 6 if geom.patch_size == 32 else 3
            patches = e.preprocess(*pack(list(W.synthetic_crops(n, seed=5))))
            emit(f"{name} defaults", *e.vit_forward(patches))
            for sw, setter, values in switches:
                for v in values[1:]:
                    setter(e, v)
                    emit(f"{name} {sw}={v}", *e.vit_forward(patches))
                setter(e, values[0])
            e.set_forward_pruning(True)
            for tok in (0, geom.seq_len - 1):
                emit(f"{name} pruned pool_token={tok}", *e.vit_forward(patches, pool_token=tok))
            emit(f"{name} tokens pruned", *e.vit_tokens(patches))
            e.set_forward_pruning(False)
            emit(f"{name} tokens defaults", *e.vit_tokens(patches))
            e.set_chunk(2)
            five = pack(list(W.synthetic_crops(5, seed=6)))
            patches = e.preprocess(*five)
            emit(f"{name} chunk=2 n=5", *e.vit_forward(patches))
            emit(f"{name} tokens chunk=2 n=5", *e.vit_tokens(patches))
            if name in ("vit_b16", "vit_b32", "dinov2_b14"):  # the pixel path, one tower per retile form
                emit(f"{name} embed chunk=2 n=5", *e.embed(*five))
                emit(f"{name} embed_tokens chunk=2 n=5", *e.embed_tokens(*five))
            e.close()

    def text():
        for proj in (512, None):
            geom = W.CLIPTextGeometry(num_layers=2, vocab_size=256, eos_token_id=255, projection_dim=proj)
            e = Engine(0)
            e.load_clip_text(W.make_clip_text_weights(41, geom), geom)
            for n in (3, 1030) if proj else (3,):  # MME_TEXT_CHUNK is 1024: a full chunk and a ragged one
                emit(f"text projection={proj} n={n}", *e.text_forward(W.synthetic_token_ids(n, geom.vocab_size, geom.eos_token_id, 7)))
            e.close()
        geom = W.SiglipTextGeometry(num_layers=2, vocab_size=256)
        e = Engine(0)
        e.load_siglip_text(W.make_siglip_text_weights(43, geom), geom)
        emit("siglip_text n=3", *e.text_forward(W.siglip_token_ids(3, geom.vocab_size, geom.pad_token_id, 7)))
        e.close()

    def tile():
        rng = np.random.default_rng(4)
        arrays = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(300, 200, 3), (1000, 1100, 3)]]
        w = None
        for point in ("after", "before"):
            geom = dataclasses.replace(W.TILE_VIT, num_layers=1, num_global_layers=1, intermediate_layers=(0,), intermediate_save_point=point)
            w = w or W.make_tile_vit_weights(3, geom)  # the tensors do not depend on the save point
            e = Engine(0)
            e.load_tile_vit(w, geom)
            pv, ids, _, nt = e.preprocess_tiles(*pack(arrays), 560, 4)
            assert nt == [1, 4], nt
            for ln in (1, 2):
                e.set_ln_fusion(ln)
                for attn in (0, 1, 2):
                    e.set_attention_mode(attn)
                    emit(f"tile save={point} ln_mode={ln} attention_mode={attn}", *e.tile_vit_forward(pv, ids, nt, want_hidden=True))
            e.close()

    def rows():
        t, dev = torch, "cuda:0"
        BF, F = t.bfloat16, t.float32
        rng = np.random.default_rng(17)
        N, IMG, TXT, PS = 5, (384, 768, 1024), (512, 768, 1024), (64, 320, 1024)

        def f32(*shape, scale=1.0, shift=0.0):
            return t.from_numpy((shift + scale * rng.standard_normal(shape)).astype(np.float32)).to(dev)

        def bf(*shape):
            return f32(*shape).to(BF)

        class Out:
            """a sentinel-filled byte buffer with 256 more bytes behind the tensor the kernel is handed"""

            def __init__(self, dtype, *shape, init=None):
                nbytes = int(np.prod(shape)) * t.empty((), dtype=dtype).element_size()
                self.raw = t.full((nbytes + 256,), 0xA5, dtype=t.uint8, device=dev)
                self.view = self.raw[:nbytes].view(dtype).view(*shape)
                if init is not None:
                    self.view.copy_(init)

        e = Engine(0)
        for d in IMG:
            x, gamma, beta = bf(N, d), f32(d, scale=0.2, shift=1.0), f32(d, scale=0.5)
            y, st = Out(BF, N, d), Out(F, N, 2)
            e.rowop_apply("layernorm", x=x, y=y.view, gamma=gamma, beta=beta, rows=N, d=d, eps=1e-12)
            emit(f"rows layernorm d={d}", y.raw)
            e.rowop_apply("ln_stats", x=x, stats=st.view, rows=N, d=d, eps=1e-12)
            emit(f"rows ln_stats d={d}", st.raw)
            xs = Out(BF, N * 197, d)
            e.rowop_apply("cls_rows", x=xs.view, cls=f32(d), pos=f32(197, d), B=N, d=d)
            emit(f"rows cls_rows d={d}", xs.raw)
            xp, st = Out(BF, N, d, init=x), Out(F, N, 2)
            e.clip_apply("pre_ln", x=xp.view, gamma=gamma, beta=beta, stats=st.view, rows=N, d=d, eps=1e-5)
            emit(f"rows pre_ln d={d}", xp.raw, st.raw)
            for tokens, pool, pool_l2 in ((197, lambda **kw: e.clip_apply("pool_ln", B=N, **kw), lambda **kw: e.rowop_apply("pool_ln_l2", B=N, **kw)),
                                          (50, lambda **kw: e.vit32_apply("pool_ln", n=N, **kw), lambda **kw: e.vit32_apply("pool_ln_l2", n=N, **kw))):
                xt = bf(N * tokens, d)
                for tok in (0, tokens - 1):
                    y, e32, e16 = Out(BF, N, d), Out(F, N, d), Out(BF, N, d)
                    pool(x=xt, gamma=gamma, beta=beta, y=y.view, tok=tok, d=d, eps=1e-5)
                    emit(f"rows pool_ln tokens={tokens} tok={tok} d={d}", y.raw)
                    pool_l2(x=xt, gamma=gamma, beta=beta, emb_f32=e32.view, emb_bf16=e16.view, tok=tok, d=d, eps=1e-12)
                    emit(f"rows pool_ln_l2 tokens={tokens} tok={tok} d={d}", e32.raw, e16.raw)
            xt = bf(N * 257, d)  # the 257-token layout has no pool_ln hook: the form with the L2 step only
            for tok in (0, 256):
                e32, e16 = Out(F, N, d), Out(BF, N, d)
                e.dinov2_apply("pool_ln_l2", x=xt, gamma=gamma, beta=beta, emb_f32=e32.view, emb_bf16=e16.view, n=N, tok=tok, d=d, eps=1e-12)
                emit(f"rows pool_ln_l2 tokens=257 tok={tok} d={d}", e32.raw, e16.raw)
            bias = f32(d)
            xo = Out(BF, 2 * 257, d)
            e.dinov2_apply("embed_rows", acc=f32(2 * 256, d), bias=bias, pos=f32(257, d), cls=f32(d), x=xo.view, n=2, d=d)
            emit(f"rows embed_rows tokens=257 d={d}", xo.raw)
            xo = Out(BF, 2 * 50, d)
            e.vit32_apply("embed_rows", acc=f32(2 * 49, d), bias=bias, pos=f32(50, d), cls=f32(d), x=xo.view, n=2, d=d)
            emit(f"rows embed_rows tokens=50 d={d}", xo.raw)
            xo = Out(BF, 2 * 196, d)
            e.siglip_apply("embed_rows", acc=f32(2 * 196, d), bias=bias, pos=f32(196, d), x=xo.view, n=2, d=d)
            emit(f"rows embed_rows tokens=196 d={d}", xo.raw)
            e32, e16 = Out(F, N, d), Out(BF, N, d)
            e.siglip_apply("l2_bf16", x=x, emb_f32=e32.view, emb_bf16=e16.view, n=N, d=d)
            emit(f"rows l2_bf16 p={d}", e32.raw, e16.raw)
        for p in PS:
            xf, bias = f32(N, p), f32(p)
            y32, y16 = Out(F, N, p), Out(BF, N, p)
            e.clip_apply("l2", xf=xf, y_f32=y32.view, y_bf16=y16.view, rows=N, p=p)
            emit(f"rows l2 p={p}", y32.raw, y16.raw)
            y32, y16 = Out(F, N, p), Out(BF, N, p)
            e.siglip_text_apply("bias_l2", acc=xf, bias=bias, emb_f32=y32.view, emb_bf16=y16.view, n=N, p=p)
            emit(f"rows bias_l2 p={p}", y32.raw, y16.raw)
        for d in TXT:
            gamma, beta = f32(d, scale=0.2, shift=1.0), f32(d, scale=0.5)
            y, yf = Out(BF, N, d), Out(F, N, d)
            e.text_apply("eos_pool_ln", x=bf(N * 77, d), gamma=gamma, beta=beta, eos_pos=[0, 1, 76, 0, 76], y=y.view, y_f32=yf.view, n=N, d=d, eps=1e-5)
            emit(f"rows eos_pool_ln tokens=77 d={d}", y.raw, yf.raw)
            y, yf = Out(BF, N, d), Out(F, N, d)
            e.siglip_text_apply("last_pool_ln", x=bf(N * 64, d), gamma=gamma, beta=beta, y=y.view, y_f32=yf.view, n=N, d=d, eps=1e-6)
            emit(f"rows last_pool_ln tokens=64 d={d}", y.raw, yf.raw)
        e.close()

    def resample():
        t, dev = torch, "cuda:0"
        rng = np.random.default_rng(23)
        shapes = [(1, 1), (20, 63), (63, 20), (300, 224), (224, 300), (100, 224), (1400, 1350), (17, 8000), (37, 1000), (2000, 3000)]
        mixed = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in (shapes[i] for i in rng.permutation(len(shapes)))]
        alone = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)]

        def out(nbytes):
            return t.full((nbytes + 256,), 0xA5, dtype=t.uint8, device=dev)

        e = Engine(0)
        # (name, mean, std, the form the patch emitter takes): tests/test_gpu_normalisation.py, "half" and "table_ch0"
        norms = [("fma", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), True), ("table", (0.6, 0.892, 0.7415), (0.1993, 0.0298, 0.0224), False)]
        for rule in ("fit_pad", "clip"):
            e.set_resize_rule(rule)
            for norm, mean, std, exact in norms:
                e.set_normalisation(mean, std)
                assert e.normalisation_form()[0] == exact, (norm, e.normalisation_form())
                for batch, arrays in (("mixed", mixed), ("224x224", alone)):
                    pix, offs, hw = pack(arrays)
                    offs, hw = e._crop_tables(offs, hw)
                    raw = out(len(arrays) * 196 * 768 * 2)
                    e._check(e.lib.mme_preprocess(e.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, len(arrays), raw.data_ptr(), e._stream()),
                             "mme_preprocess")
                    emit(f"resample preprocess rule={rule} norm={norm} batch={batch}", raw)
        e.set_resize_rule("fit_pad")
        pix, offs, hw = pack(mixed)
        offs, hw = e._crop_tables(offs, hw)
        n, tile, max_tiles = len(mixed), 560, 4
        raw = out(n * max_tiles * 3 * tile * tile * 4)
        ids, nt = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        e._check(e.lib.mme_preprocess_tiles(e.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, tile, max_tiles, raw.data_ptr(), ids.ctypes.data,
                                            nt.ctypes.data, e._stream()), "mme_preprocess_tiles")
        emit("resample preprocess_tiles tile=560 max_tiles=4", raw, t.from_numpy(np.concatenate([ids, nt])))
        # (source h, w, new_h, new_w): an ordinary cap with a ragged last tile on both axes, and the vertical-first order
        for name, (h, w, nh, nw) in (("ordinary", (700, 1303, 431, 803)), ("vertical_first", (2300, 21, 1237, 13))):
            src = t.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)
            raw = out(nh * nw * 3)
            e.lanczos_resize(src, nh, nw, out=raw[: nh * nw * 3])
            emit(f"resample lanczos_resize {name} {h}x{w}->{nh}x{nw}", raw)
        e.close()

    for name, fn in (("image", image), ("text", text), ("tile", tile), ("rows", rows), ("resample", resample)):
        if args.only in (None, name):
            fn()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
