#!/usr/bin/env python3
"""Timing of the 8000-pixel cap on seeded oversized pages; raw lines go to profiles/lanczos_cap.txt.

    python tools/bench_cap.py [--sizes 9000x12000,16000x12000]        (width x height)

Per page, one JSON line with
  pillow_s        Image.resize(..., Image.LANCZOS) on the host: median and range of 3
  device_s        Engine.lanczos_resize alone, pixels already on the device: 2 warm-up calls, then median and range of 7
                  synchronous calls (host table build and upload included: they are part of every call)
  bytes, tb_per_s the bytes the two kernels move (source read, scratch image written and read, output written) over the
                  median, beside the 5.5 TB/s stream rate K1 reaches
  e2e_host_s      get_image_embeddings([page]) with the cap on the host (the path before the device cap), page upload
                  included: median and range of 3
  e2e_device_s    the same call with the cap on the device: 1 warm-up call, median and range of 3
and `equal`: the device result equals Pillow's, byte for byte.  No figure is gated.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 6), "min": round(v[0], 6), "max": round(v[-1], 6)}


def timed(fn, runs, sync=None):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        out.append(time.perf_counter() - t0)
    return stats(out)


def main():
    import torch
    from PIL import Image

    from multimodal_embeddings_amd import embedder as E

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="9000x12000,16000x12000")
    args = ap.parse_args()
    emb = E.RegionEmbedder()
    eng = emb.engine
    sync = torch.cuda.synchronize
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        page = np.random.default_rng(w * 31 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw = E.capped_size(h, w)
        img = Image.fromarray(page)
        want = []
        pillow = timed(lambda: want.append(np.asarray(img.resize((nw, nh), Image.LANCZOS))), 3)
        dpage = torch.from_numpy(page).cuda()
        work = torch.empty(E.lanczos_workspace(h, w, nh, nw), dtype=torch.uint8, device="cuda")
        out = torch.empty(nh * nw * 3, dtype=torch.uint8, device="cuda")
        call = lambda: eng.lanczos_resize(dpage, nh, nw, out=out, work=work)  # noqa: E731
        timed(call, 2, sync)
        device = timed(call, 7, sync)
        equal = bool(np.array_equal(out.view(nh, nw, 3).cpu().numpy(), want[0]))
        pitch = (nw * 3 + 15) // 16 * 16
        moved = h * w * 3 + 2 * h * pitch + nh * nw * 3
        del dpage, work, out
        real = E._load_for_device
        E._load_for_device = E._load_rgb  # the cap on the host, as before
        try:
            e2e_host = timed(lambda: emb.get_image_embeddings([page]), 3)
        finally:
            E._load_for_device = real
        emb.get_image_embeddings([page])
        e2e_device = timed(lambda: emb.get_image_embeddings([page]), 3)
        print(json.dumps({"page_wxh": [w, h], "capped_wxh": [nw, nh], "pillow": Image.__version__, "pillow_s": pillow, "device_s": device, "bytes": moved,
                          "tb_per_s": round(moved / device["median"] / 1e12, 4), "k1_stream_tb_per_s": 5.5, "e2e_host_s": e2e_host,
                          "e2e_device_s": e2e_device, "equal": equal}), flush=True)


if __name__ == "__main__":
    main()
