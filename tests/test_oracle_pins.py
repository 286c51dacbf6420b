"""The oracle is only trusted once it reproduces every golden vector (tier rule 3).

Goldens come from tests/golden/make_golden.py: the reference's own functions
(cluster_images, compute_image_similarity_matrix, last_pooling), its bundled report
and data files, and the third-party code it delegates to (transformers ViT / Mllama
image processor, Pillow, scipy, scikit-learn).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from multimodal_embeddings_amd.weights import make_vit_weights, synthetic_crops
from oracle import cluster as oc
from oracle import compare as ocmp
from oracle import preprocess as opre
from oracle import vit as ovit


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_report_kat_labels(golden_dir):
    rep = json.load(open(os.path.join(golden_dir, "report_matrix.json")))
    M = np.array(rep["matrix"])
    res = oc.cluster_images(M.copy(), list(rep["names"]))
    assert res["n_clusters"] == rep["n_clusters"] == 10
    assert res["labels"] == rep["labels"] == [7, 9, 0, 5, 0, 4, 0, 0, 0, 0, 2, 2, 2, 8, 0, 3, 6, 0, 1]
    for k, v in rep["cohesion"].items():
        assert res["cluster_cohesion"][int(k)] == pytest.approx(v, abs=1e-15)
    # fallback-path silhouettes for k=2..10
    D = 1.0 - M
    np.fill_diagonal(D, 0.0)
    want = [-0.2596, -0.2582, -0.2045, -0.1714, -0.1720, -0.1716, -0.1430, -0.1420, -0.1250]
    got = [oc.silhouette_precomputed(D, oc.agglomerative_labels(D, k)) for k in range(2, 11)]
    assert np.allclose(got, want, atol=5e-5)
    # precomputed mode gives the OTHER labelling the survey probed (G3)
    pre = oc.cluster_images(M.copy(), list(rep["names"]), mode="precomputed")
    assert pre["labels"] != rep["labels"]


def test_cluster_cases_match_reference(golden_dir):
    g = _load(golden_dir, "cluster_cases.npz")
    n = int(g["n_cases"])
    assert n >= 15
    for c in range(n):
        S = g[f"c{c}_S"]
        fixed = int(g[f"c{c}_fixed"])
        names = [f"page_{i:03d}.png" for i in range(S.shape[0])]
        if f"c{c}_none" in g:
            with pytest.raises(Exception):
                r = oc.cluster_images(S.copy(), names, n_clusters=None if fixed < 0 else fixed)
                assert r is not None
            continue
        r = oc.cluster_images(S.copy(), names, n_clusters=None if fixed < 0 else fixed)
        assert r["labels"] == g[f"c{c}_labels"].tolist(), c
        assert r["n_clusters"] == int(g[f"c{c}_k"]), c
        keys = g[f"c{c}_coh_keys"].tolist()
        assert sorted(r["cluster_cohesion"]) == keys
        assert np.allclose([r["cluster_cohesion"][k] for k in keys], g[f"c{c}_coh_vals"], rtol=0, atol=1e-15)


def test_linkage_matches_scipy_and_sklearn(golden_dir):
    g = _load(golden_dir, "linkage_cases.npz")
    tags = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_D")})
    assert tags
    for t in tags:
        D = g[t + "_D"]
        P = D.shape[0]
        Z = oc.linkage_average(oc.pdist_rows_euclidean(D), P)
        assert np.array_equal(Z[:, :2], g[t + "_Z"][:, :2]), t
        assert np.allclose(Z[:, 2], g[t + "_Z"][:, 2], rtol=1e-15, atol=0), t
        assert np.array_equal(Z[:, 3], g[t + "_Z"][:, 3]), t
        Zp = oc.linkage_average(oc.squareform_to_condensed(D), P)
        assert np.array_equal(Zp[:, :2], g[t + "_Zpre"][:, :2]), t
        for k in range(2, min(10, P) + 1):
            assert np.array_equal(oc.agglomerative_labels(D, k), g[f"{t}_lab{k}"]), (t, k)
            assert np.array_equal(oc.agglomerative_labels(D, k, "precomputed"), g[f"{t}_labpre{k}"]), (t, k)
            if f"{t}_sil{k}" in g:
                assert oc.silhouette_precomputed(D, g[f"{t}_lab{k}"]) == pytest.approx(float(g[f"{t}_sil{k}"]), abs=1e-14)


def test_pagesim_matches_reference(golden_dir):
    g = _load(golden_dir, "pagesim_cases.npz")
    pages = json.load(open(os.path.join(golden_dir, "region_table.json")))
    names = [p["name"] for p in pages]
    for metric in ("cosine", "sqeuclidean"):
        S, nm = ocmp.compute_image_similarity_matrix(g["real_emb"], g["real_area_percentage"], g["real_page_of"], names, metric=metric)
        assert nm == names
        assert np.allclose(S, g[f"real_S_{metric}"], rtol=1e-12, atol=1e-15)
    S, _ = ocmp.compute_image_similarity_matrix(g["real_emb"], g["real_area_percentage"], g["real_page_of"], names, skip_same_prefix=False)
    assert np.allclose(S, g["real_S_cosine_noskip"], rtol=1e-12, atol=1e-15)
    syn_names = json.load(open(os.path.join(golden_dir, "pagesim_names.json")))["names"]
    types = ["plain_text" if ok else "abandon" for ok in g["syn_types_ok"]]
    for metric in ("cosine", "sqeuclidean"):
        S, _ = ocmp.compute_image_similarity_matrix(g["syn_emb"], g["syn_area_percentage"], g["syn_page_of"], syn_names, types, metric=metric)
        assert np.allclose(S, g[f"syn_S_{metric}"], rtol=1e-12, atol=1e-15)
        assert S[2, 3] == 0 and S[4].sum() == 1.0  # same-prefix pair skipped, empty page only has its diagonal


def _bf16_rows(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def test_pagesim_on_bf16_rows_matches_reference(golden_dir):
    """The fixture the GPU page matrix is held to (test_gpu_parity): the REAL functions fed the bf16-rounded rows the
    device table holds, inner products of the stored rows as the collection's cosine.  The oracle agrees with it on
    the same numbers (1e-12), labels of the REAL cluster_images included."""
    from oracle import cluster as oclu

    g = _load(golden_dir, "pagesim_bf16_cases.npz")
    pages = json.load(open(os.path.join(golden_dir, "region_table.json")))
    names = [p["name"] for p in pages]
    e = _bf16_rows(g["real_emb_bf16"]).astype(np.float64)
    for metric in ("cosine", "sqeuclidean"):
        S, _ = ocmp.compute_image_similarity_matrix(None, g["real_area_percentage"], g["real_page_of"], names, metric=metric, sim=e @ e.T)
        assert np.allclose(S, g[f"real_S_{metric}"], rtol=1e-12, atol=1e-15)
        res = oclu.cluster_images(g[f"real_S_{metric}"].copy(), names)
        assert res["labels"] == g[f"real_labels_{metric}"].tolist() and res["n_clusters"] == int(g[f"real_k_{metric}"])
    syn_names = json.load(open(os.path.join(golden_dir, "pagesim_bf16_names.json")))["names"]
    e = _bf16_rows(g["syn_emb_bf16"]).astype(np.float64)
    S, _ = ocmp.compute_image_similarity_matrix(None, g["syn_area_percentage"], g["syn_page_of"], syn_names, sim=e @ e.T)
    assert np.allclose(S, g["syn_S_cosine"], rtol=1e-12, atol=1e-15)
    res = oclu.cluster_images(g["syn_S_cosine"].copy(), syn_names)
    assert res["labels"] == g["syn_labels_cosine"].tolist()


def test_pagesim_empty_table():
    assert ocmp.compute_image_similarity_matrix(np.zeros((0, 8)), np.zeros(0), np.zeros(0, dtype=int), ["a", "b"]) == (None, None)


def test_region_table_counts(golden_dir):
    pages = json.load(open(os.path.join(golden_dir, "region_table.json")))
    assert len(pages) == 19
    nbox = sum(len(p["boxes"]) for p in pages)
    nemb = sum(sum(c in ocmp.REGION_TYPES_TO_PROCESS for c in p["class_names"]) for p in pages)
    assert (nbox, nemb) == (1938, 1867)
    for p in pages:  # detector-score order (G6)
        assert all(a >= b for a, b in zip(p["scores"], p["scores"][1:]))


def test_last_pooling_matches_reference(golden_dir):
    g = _load(golden_dir, "last_pooling.npz")
    hs, mask = torch.from_numpy(g["hs"]), torch.from_numpy(g["mask"])
    assert np.array_equal(ovit.last_pooling(hs, mask).numpy(), g["out"])
    assert np.array_equal(ovit.last_pooling(hs, mask, normalize=False).numpy(), g["out_raw"])


def test_vit_matches_transformers(golden_dir):
    g = _load(golden_dir, "vit_cases.npz")
    crops = synthetic_crops(int(g["n"]), seed=int(g["crop_seed"]))
    patches = np.stack([opre.preprocess_to_patches(c) for c in crops])
    for tag, std in (("std002", 0.02), ("std008", 0.08)):
        w = make_vit_weights(seed=1, std=std)
        hs = ovit.vit_hidden_states(torch.from_numpy(patches), w).numpy()
        assert np.abs(hs[:, ::49, ::64] - g[f"{tag}_hidden_sample"]).max() < 2e-4
        for pool in ("cls", "last"):
            e = ovit.vit_embed(patches, w, pool=pool)
            cos = np.sum(e * g[f"{tag}_{pool}"], axis=1)
            assert np.all(1.0 - cos < 1e-6), (tag, pool, cos)


def test_preprocess_matches_pillow_and_mllama_processor(golden_dir):
    from PIL import Image

    man = json.load(open(os.path.join(golden_dir, "crops_manifest.json")))
    g = _load(golden_dir, "crops_expected.npz")
    assert man["c1_count"] == 16
    for i, c in enumerate(man["crops"]):
        img = np.array(Image.open(os.path.join(golden_dir, "crops", c["file"])).convert("RGB"))
        assert img.shape[:2] == (c["height"], c["width"])
        assert opre.fit_to_canvas(c["height"], c["width"]) == (c["new_h"], c["new_w"])
        rs = opre.pil_bilinear_resize_u8(img, c["new_h"], c["new_w"])
        assert np.array_equal(rs, g[f"resized_{i}"]), c["file"]
        pv = opre.preprocess_crop(img)
        assert np.array_equal(pv[:, ::7, ::5], g[f"pv_sample_{i}"])
        sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(pv).tobytes()).digest(), dtype=np.uint8)
        assert np.array_equal(sha, g[f"pv_sha256_{i}"]), c["file"]


def test_resize_matches_live_pillow_on_synthetic_shapes():
    """Pillow is in the image on both boxes: compare live on shapes the fixtures do not hold."""
    from PIL import Image

    rng = np.random.default_rng(5)
    for h, w in [(20, 63), (5114, 60), (37, 3862), (224, 224), (223, 225), (1, 500), (300, 1), (448, 448), (100, 100), (1000, 333)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw = opre.fit_to_canvas(h, w)
        ref = np.array(Image.fromarray(img).resize((nw, nh), resample=Image.BILINEAR))
        assert np.array_equal(opre.pil_bilinear_resize_u8(img, nh, nw), ref), (h, w)


def test_bundled_crop_sizes_equal_int_bbox(golden_dir):
    """every bundled crop's pixel size equals the int()-truncated bbox.  The crops' file names and
    (height, width) are data fixtures (bundled_crop_names.json, bundled_crop_sizes_hw.npy, both in sorted-name order),
    read by make_golden.py off the reference's output/region_images."""
    pages = json.load(open(os.path.join(golden_dir, "region_table.json")))
    names = json.load(open(os.path.join(golden_dir, "bundled_crop_names.json")))
    hw = np.load(os.path.join(golden_dir, "bundled_crop_sizes_hw.npy"))
    size = {f: (int(w), int(h)) for f, (h, w) in zip(names, hw)}
    assert len(size) == len(names) == len(hw) == 1862
    checked = 0
    for p in pages:
        stem = os.path.splitext(p["name"])[0]
        for i, (box, cname) in enumerate(zip(p["boxes"], p["class_names"])):
            f = f"{stem}_region{i}_{cname}.png"
            if f not in size:
                continue
            x0, y0, x1, y1 = opre.crop_box_int(box)
            assert size[f] == (x1 - x0, y1 - y0)
            checked += 1
    assert checked == 1862


def _pin_crops(crops):
    """worker: oracle.preprocess_crop vs transformers' Mllama processor (live) on a slice of the crops; a crop is a PNG
    path or (index, height, width) of seeded synthetic pixels"""
    from PIL import Image
    from threadpoolctl import threadpool_limits
    from transformers.models.mllama.image_processing_pil_mllama import MllamaImageProcessorPil

    threadpool_limits(1)  # one BLAS thread per worker: the pool is the parallelism
    proc = MllamaImageProcessorPil(size={"height": 224, "width": 224}, max_image_tiles=1, image_mean=list(opre.CLIP_MEAN),
                                   image_std=list(opre.CLIP_STD))
    bad = []
    for c in crops:
        if isinstance(c, str):
            im, label = Image.open(c), os.path.basename(c)
        else:
            k, h, w = c
            im, label = Image.fromarray(np.random.default_rng([7, k]).integers(0, 256, (h, w, 3), dtype=np.uint8)), f"shape {k}: {h} x {w}"
        want = proc(images=[im], return_tensors="np")["pixel_values"][0, 0, 0]
        a = np.array(im.convert("RGB"))
        nh, nw = opre.fit_to_canvas(*a.shape[:2])
        if not (np.array_equal(opre.preprocess_crop(a), want)
                and np.array_equal(opre.pil_bilinear_resize_u8(a, nh, nw), np.array(im.convert("RGB").resize((nw, nh), resample=Image.BILINEAR)))):
            bad.append(label)
    return len(crops), bad


def test_oracle_preprocessing_is_bit_exact_on_every_bundled_crop(golden_dir):
    """north_star: "on the bundled newspaper_images set".  oracle.preprocess_crop / pil_bilinear_resize_u8 against live
    Pillow and live transformers MllamaImageProcessorPil: bit-exact f32 pixel values and bit-exact resized bytes, on
    every one of the 1862 bundled crop shapes (bundled_crop_sizes_hw.npy, seeded synthetic pixels: the crops themselves
    are 178 MB) and on the committed bundled crops (tests/golden/crops) as they are.
    (The GPU-side K1 check uses the committed crops plus the bundled size distribution; this pins the checker.)"""
    import multiprocessing as mp

    hw = np.load(os.path.join(golden_dir, "bundled_crop_sizes_hw.npy"))
    assert len(hw) == 1862
    crop_dir = os.path.join(golden_dir, "crops")
    files = sorted(os.path.join(crop_dir, f) for f in os.listdir(crop_dir) if f.endswith(".png"))
    assert len(files) == 24
    crops = files + [(k, int(h), int(w)) for k, (h, w) in enumerate(hw)]
    workers = 6
    parts = [crops[k::workers] for k in range(workers)]
    with mp.get_context("fork").Pool(workers) as pool:
        results = pool.map(_pin_crops, parts)
    assert sum(n for n, _ in results) == len(crops)
    assert [b for _, bad in results for b in bad] == []


def test_neighbour_lists_match_reference_region_report(golden_dir):
    """oracle.neighbour_lists == what create_region_cross_comparison (region_compare.py:25) picked on a
    brute-force store: ranks, same-page / self drops, the literal distance >= 0.3 window (G2)."""
    from oracle import compare as oc

    g = np.load(os.path.join(golden_dir, "neighbour_cases.npz"))
    emb, page, area = g["region_emb"], g["region_page"], g["region_area"]
    idx, sim, w = oc.neighbour_lists(emb, page, top_n=10, area_percentage=area, max_sim=1.0 - 0.3)
    want_idx, want_d = g["region_idx"].copy(), g["region_distance"]
    no_box = int(g["region_no_box"][0])
    assert (want_idx[no_box] == -1).all()  # the reference skips it as a source (:147-149)
    rows = [r for r in range(len(emb)) if r != no_box]
    assert np.array_equal(idx[rows], want_idx[rows])
    got_d = np.where(idx >= 0, 1.0 - sim, 0.0)
    assert np.abs(got_d[rows] - want_d[rows]).max() < 1e-12
    # every picked distance is >= 0.3 although nearer neighbours exist: the inverted threshold of G2
    assert want_d[want_idx >= 0].min() >= 0.3 and (1.0 - oc.cosine_matrix(emb)[5, 60]) < 1e-12 and 60 not in want_idx[5]
    # weighted score of :273-278 (on the similarity here; the reference multiplies its distance)
    r, c = rows[0], idx[rows[0], 0]
    assert w[r, 0] == sim[r, 0] * (area[r] / 100.0) * (area[c] / 100.0)


def test_image_neighbour_lists_match_reference_cross_compare(golden_dir):
    """oracle.image_neighbour_lists == the picks create_cross_comparison (cross_compare.py:19) wrote
    into its HTML pages (source-dependent 20 % filename prefix rule), scores at the 4 printed decimals."""
    from oracle import compare as oc

    g = np.load(os.path.join(golden_dir, "neighbour_cases.npz"))
    names = json.load(open(os.path.join(golden_dir, "neighbour_names.json")))["image_names"]
    lists = oc.image_neighbour_lists(oc.cosine_matrix(g["image_emb"]), names, top_n=5)
    want_idx, want_d = g["image_idx"], g["image_distance_4dp"]
    for r, lst in enumerate(lists):
        k = len(lst)
        assert [c for c, _ in lst] == want_idx[r, :k].tolist() and (want_idx[r, k:] == -1).all(), r
        assert all(abs(round(1.0 - s, 4) - want_d[r, j]) < 1e-9 for j, (_, s) in enumerate(lst))
    assert all(len(l) == 5 for l in lists)
    # the 7-character prefix of an 'Addison NY Advertiser 1883' page excludes the 1884 pages too
    assert all(not names[c].startswith("Addison") for c, _ in lists[0])


def test_region_rows_and_crops_match_reference_region_processor(golden_dir):
    """oracle.regions == what RegionProcessor.process_image_regions (region_processor.py:62) upserted and the
    crops the real get_region_image (doclayout_detector.py:165) handed to the embedder -- fractional, edge
    and partly-outside boxes, one class that is not embedded."""
    from oracle import regions as oreg

    g = json.load(open(os.path.join(golden_dir, "region_rows.json")))
    H, W = g["page_hw"]
    page = np.random.default_rng(g["seed"]).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ids, metas, docs = oreg.region_rows("<page_path>/" + g["page_name"], g["regions"])
    assert ids == g["ids"] and docs == g["documents"] and len(ids) == 7
    for got, want in zip(metas, g["metadatas"]):
        got = dict(got, parent_image="<page_path>")
        assert got == want  # every key, floats bit-equal (area_percentage, box_normalized strings)
    kept = [b for b, c in zip(g["regions"]["boxes"], g["regions"]["class_names"]) if c in oreg.REGION_TYPES_TO_PROCESS]
    for box, shape, sha in zip(kept, g["crop_shapes"], g["crop_sha256"]):
        crop = oreg.crop_region(page, box)
        assert list(crop.shape) == shape and hashlib.sha256(crop.tobytes()).hexdigest() == sha


def test_nms_oracle_keeps_what_the_reference_function_kept(golden_dir):
    """oracle.regions.nms_keep == the indices the REAL apply_non_max_suppression (3_combine_grids.py:80-137) kept, in its
    output order: the boxes of the 19 bundled pages at four thresholds (idempotent at the 0.5 they were produced with) and
    seeded box sets with equal scores, duplicates, boxes sharing an edge and zero-width boxes."""
    from oracle import regions as oreg

    cases = json.load(open(os.path.join(golden_dir, "nms_cases.json")))["cases"]
    assert len(cases) >= 27 and sum(len(c["scores"]) for c in cases) > 5000
    for c in cases:
        for run in c["runs"]:
            assert oreg.nms_keep(c["boxes"], c["scores"], c["classes"], run["iou_threshold"]) == run["keep"], (c["name"], run["iou_threshold"])
    # calculate_iou's branches: disjoint -> 0, shared edge -> 0 through the area branch, zero-area pair -> 0, identical -> 1
    assert oreg.box_iou([0, 0, 10, 10], [[20, 0, 30, 10], [10, 0, 20, 10], [0, 0, 10, 10], [0, 0, 5, 10]]).tolist() == [0.0, 0.0, 1.0, 0.5]
    assert oreg.box_iou([1, 1, 1, 1], [[1, 1, 1, 1]]).tolist() == [0.0]


def test_tile_preprocessing_matches_transformers_mllama_processor(golden_dir):
    """oracle.preprocess_tiles == transformers' MllamaImageProcessorPil at the checkpoint geometry (tile 560,
    <= 4 tiles): canvas choice, aspect-ratio id / mask, tile count, and every f32 pixel value (sha256) on the
    committed crops and on seeded arrays that reach all eight tile arrangements."""
    from PIL import Image

    g = json.load(open(os.path.join(golden_dir, "tile_cases.json")))
    probe = np.array(g["probe_index"])
    seen = set()
    for c in g["cases"]:
        kind, rest = c["source"].split(":", 1)
        if kind == "file":
            img = np.array(Image.open(os.path.join(golden_dir, "crops", rest)).convert("RGB"))
        else:
            seed, hw = rest.split(":")
            h, w = map(int, hw.split("x"))
            img = np.random.default_rng(int(seed)).integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert list(img.shape[:2]) == c["hw"]
        pv, aid, nt, (th, tw) = opre.preprocess_tiles(img, g["tile"], g["max_tiles"])
        assert aid == c["aspect_ratio_id"] and nt == c["num_tiles"] == th * tw
        assert [1] * nt + [0] * (g["max_tiles"] - nt) == c["aspect_ratio_mask"]
        assert pv.reshape(-1)[probe].tolist() == c["probe"]
        assert hashlib.sha256(np.ascontiguousarray(pv).tobytes()).hexdigest() == c["sha256"], c["source"]
        seen.add(aid)
    assert seen == set(range(1, 9))
