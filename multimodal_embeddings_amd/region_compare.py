"""Ranked "similar regions from other pages" lists -- the data of the reference's region report.

Mirrors `create_region_cross_comparison` (deprecated_package/region_compare.py:25-406) without
its HTML / cv2 output (emit JSON instead): the per-region store query
(:165-170) plus the filter loop (:238-353) run as ONE pass of the K12 kernel
(`mme_neighbours`: MFMA cosine block + streaming top-k) over every region at once.

`duplicate_groups` answers the question a ranking cannot: which regions are the same thing printed again (a syndicated
advertisement, a masthead, a reprinted notice) -- the connected components of "cosine >= threshold between regions of
different pages" over all regions at once (kernel K14, `mme_duplicates_*`), and which pages share such regions.
"""
from __future__ import annotations

import dataclasses
import json
import logging
import os

import numpy as np

from . import config
from ._lib import Engine
from .cross_compare import default_engine, to_unit_bf16

logger = logging.getLogger(__name__)


def _box_of(meta):
    """region_compare.py:133-146: box from `box_str` or the four box_* keys, else None."""
    if meta.get("box_str"):
        return [float(x) for x in meta["box_str"].split(",")]
    keys = ["box_x_min", "box_y_min", "box_x_max", "box_y_max"]
    if all(k in meta for k in keys):
        return [meta[k] for k in keys]
    return None


def region_neighbours(collection, top_n=config.REGION_COMPARE_TOP_N, *, score="cosine",
                      threshold=config.REGION_SIMILARITY_THRESHOLD, weight_by_area=config.WEIGHT_BY_AREA,
                      engine: Engine | None = None, rows: tuple[int, int] | None = None):
    """For every region of the collection: its `top_n` most similar regions from other pages.

    collection: anything with chroma's `.get(include=[...], where={"is_region": {"$eq": True}})`
    (region_compare.py:51-54).  `score`:
      * "cosine" (default) -- score = cosine similarity, regions scoring below `threshold` are
        dropped: what :266-270 means to do;
      * "reference_distance" -- score = the store's cosine DISTANCE, dropped when below
        `threshold`: what :266-270 literally executes.
    `rows=(row0, nrows)` restricts the source regions (one shard per GPU); candidates are always
    all regions.  Returns a list of dicts, one per source region that has the metadata the
    reference requires (:150-152), in collection order:
      {"id", "parent_image", "type", "area_percentage",
       "similar_regions": [{"id", "score", "weighted_score", "parent_image", "type"}, ...]}   (:340-346)
    """
    if score not in ("cosine", "reference_distance"):
        raise ValueError("score must be 'cosine' or 'reference_distance'")
    all_entries = collection.get(include=["metadatas", "embeddings", "documents"], where={"is_region": {"$eq": True}})
    if not all_entries or not all_entries.get("ids"):
        logger.warning("No regions found in the database. Make sure regions have been processed first.")  # :56-58
        return []
    ids, metas = all_entries["ids"], all_entries["metadatas"]
    n = len(ids)
    engine = engine or default_engine()
    emb = to_unit_bf16(all_entries["embeddings"], engine)

    def parent_of(m):
        return (m or {}).get("parent_image") or (m or {}).get("parent_image_name") or ""

    # group id = parent page; a row without one never equals another row's parent (:257-261)
    gid, group = {}, np.empty(n, dtype=np.int32)
    for r, m in enumerate(metas):
        p = parent_of(m)
        group[r] = gid.setdefault(p, len(gid)) if p else -(r + 1)
    row0, nrows = (0, n) if rows is None else rows
    window = {"min_sim": float(threshold)} if score == "cosine" else {"max_sim": float(1.0 - threshold)}
    idx, sim = engine.neighbours(emb, group, row0=row0, nrows=nrows, fetch=min(top_n * 3, 100), top_n=top_n, **window)
    idx, sim = idx.cpu().numpy(), sim.cpu().numpy().astype(np.float64)

    out = []
    for o in range(nrows):
        r = row0 + o
        meta = metas[r]
        if not meta:
            logger.warning(f"Missing metadata or embedding for region {ids[r]}")  # :123-125
            continue
        parent, rtype = parent_of(meta), meta.get("region_type")
        if not parent or not rtype or not _box_of(meta):
            logger.warning(f"Missing essential metadata for region {ids[r]}")  # :150-152
            continue
        area = meta.get("area_percentage", 0)
        similar = []
        for c, s in zip(idx[o], sim[o]):
            if c < 0:
                break
            cm = metas[c] or {}
            sc = float(s) if score == "cosine" else float(1.0 - s)
            weighted = sc * (area / 100) * (cm.get("area_percentage", 0) / 100) if weight_by_area else sc  # :273-280
            similar.append({"id": ids[c], "score": sc, "weighted_score": weighted,
                            "parent_image": os.path.basename(parent_of(cm)), "type": cm.get("region_type", "unknown")})
        out.append({"id": ids[r], "parent_image": os.path.basename(parent), "type": rtype, "area_percentage": area,
                    "similar_regions": similar})
    return out


def create_region_cross_comparison(collection, top_n=config.REGION_COMPARE_TOP_N, output_path=None, **kwargs):
    """Same entry point as region_compare.py:25; writes one JSON document instead of HTML pages."""
    result = region_neighbours(collection, top_n, **kwargs)
    if output_path:
        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            json.dump({"top_n": top_n, "regions": result}, fh, indent=1)
    return result


def _parent_of(m):
    return (m or {}).get("parent_image") or (m or {}).get("parent_image_name") or ""


def group_table(labels, degree, best_idx, best_sim, ids, metadatas, *, threshold=None, min_size=2, page_pairs=None, image_names=None,
                edges=None, edge_sim=None, n_edges=None):
    """The JSON-ready report from K14's arrays; a pure function of its arguments (no GPU).

    labels[i] = smallest row of row i's component, degree[i] = edges at the row, (best_idx, best_sim)[i] = its most similar
    partner or (-1, 0); ids / metadatas are the rows'.  Components of fewer than `min_size` rows are left out.  Returns
      {"threshold", "n_regions", "n_edges",
       "groups": [{"size", "pages": [page names, sorted], "members": [{"id", "parent_image", "type", "area_percentage", "degree",
                   "best_match": {"id", "score"} or None}, ... in row order]}, ... by size descending, then first member],
       "page_overlap": {"image_names", "counts"} when page_pairs is given,
       "edges": {"pairs": [{"a", "b", "score"}, ... sorted by (a, b), a < b as ids], "truncated"} when an edge list is given}
    n_edges: the number of edges found (default: sum(degree) / 2); an edge list shorter than that is flagged `truncated`."""
    labels, degree, best_idx = (np.asarray(v).astype(np.int64) for v in (labels, degree, best_idx))
    best_sim = np.asarray(best_sim, dtype=np.float64)
    n = len(ids)
    if not (len(labels) == len(degree) == len(best_idx) == len(best_sim) == len(metadatas) == n):
        raise ValueError("group_table: labels, degree, best_idx, best_sim, ids and metadatas must have one entry per row")
    members = {}
    for r in range(n):
        members.setdefault(int(labels[r]), []).append(r)
    groups = []
    for first, rows in sorted(members.items(), key=lambda kv: (-len(kv[1]), kv[0])):
        if len(rows) < max(1, int(min_size)):
            continue
        out_rows = []
        for r in rows:
            m = metadatas[r] or {}
            b = int(best_idx[r])
            out_rows.append({"id": ids[r], "parent_image": os.path.basename(_parent_of(m)), "type": m.get("region_type", "unknown"),
                             "area_percentage": m.get("area_percentage", 0), "degree": int(degree[r]),
                             "best_match": {"id": ids[b], "score": float(best_sim[r])} if b >= 0 else None})
        groups.append({"size": len(rows), "pages": sorted({m["parent_image"] for m in out_rows if m["parent_image"]}), "members": out_rows})
    total = int(degree.sum() // 2) if n_edges is None else int(n_edges)
    out = {"threshold": None if threshold is None else float(threshold), "n_regions": n, "n_edges": total, "groups": groups}
    if page_pairs is not None:
        out["page_overlap"] = {"image_names": list(image_names or []), "counts": np.asarray(page_pairs).astype(np.int64).tolist()}
    if edges is not None:
        pairs = []
        for (a, b), sc in zip(np.asarray(edges).reshape(-1, 2).tolist(), np.asarray(edge_sim, dtype=np.float64).tolist()):
            x, y = sorted((ids[a], ids[b]))
            pairs.append({"a": x, "b": y, "score": float(sc)})
        pairs.sort(key=lambda e: (e["a"], e["b"]))
        out["edges"] = {"pairs": pairs, "truncated": len(pairs) < total}
    return out


def duplicate_inputs(metadatas, exclude="parent", prefix_length=config.PREFIX_LENGTH):
    """(group int32[n] or None, page_of int32[n], image_names) of K14 from the rows' metadata; a pure function.

    exclude = "parent": regions of one page are never an edge; "prefix": neither are regions of pages whose file names share
    their first `prefix_length` characters (scans of one issue); "none": every pair counts.  A row without a parent gets a
    negative group id of its own and page -1 (not counted in the page overlap)."""
    if exclude not in ("parent", "prefix", "none"):
        raise ValueError("exclude must be 'parent', 'prefix' or 'none'")
    n = len(metadatas)
    names, page_id, page_of = [], {}, np.empty(n, dtype=np.int32)
    gid, group = {}, np.empty(n, dtype=np.int32)
    for r, m in enumerate(metadatas):
        p = os.path.basename(_parent_of(m))
        if p and p not in page_id:
            page_id[p] = len(names)
            names.append(p)
        page_of[r] = page_id[p] if p else -1
        key = p if exclude == "parent" else p[: min(int(prefix_length), len(p))]
        group[r] = gid.setdefault(key, len(gid)) if key else -(r + 1)
    return (None if exclude == "none" else group), page_of, names


def duplicate_groups(collection, threshold, *, exclude="parent", prefix_length=config.PREFIX_LENGTH, min_size=2, max_edges=0,
                     engine: Engine | None = None):
    """Groups of near-duplicate regions: the connected components of "cosine >= threshold" between the regions of the
    collection (`where={"is_region": ...}`, rows without an embedding left out), pairs chosen by `exclude` (duplicate_inputs)
    never counting.  One pass of kernel K14 over all regions; returns group_table's dict.

    `threshold` has no default: the right value belongs to the encoder.  `page_overlap` counts, per pair of pages, the edges
    between them (left out beyond 4096 pages); `max_edges` > 0 adds the edges themselves, up to that many."""
    all_entries = collection.get(include=["metadatas", "embeddings", "documents"], where={"is_region": {"$eq": True}})
    have = [r for r, e in enumerate((all_entries or {}).get("embeddings") or []) if e is not None and len(e) > 0]
    if not have:
        logger.warning("No regions found in the database. Make sure regions have been processed first.")
        return group_table([], [], [], [], [], [], threshold=threshold, min_size=min_size)
    ids = [all_entries["ids"][r] for r in have]
    metas = [all_entries["metadatas"][r] for r in have]
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)
    group, page_of, names = duplicate_inputs(metas, exclude, prefix_length)
    pages = len(names) if 1 <= len(names) <= 4096 else 0
    res = engine.duplicates(emb, group, page_of if pages else None, pages, min_sim=float(threshold), edge_cap=int(max_edges))
    host = {k: v.cpu().numpy() for k, v in res.items()}
    written = int(host["counters"][1])
    return group_table(host["labels"], host["degree"], host["best_idx"], host["best_sim"], ids, metas, threshold=threshold, min_size=min_size,
                       page_pairs=host.get("page_pairs"), image_names=names if pages else None,
                       edges=host["edges"][:written] if max_edges > 0 else None, edge_sim=host["edge_sim"][:written] if max_edges > 0 else None,
                       n_edges=int(host["counters"][0]))


def create_duplicate_report(collection, threshold, output_path=None, **kwargs):
    """duplicate_groups, written as one JSON document when `output_path` is given (as create_region_cross_comparison)."""
    result = duplicate_groups(collection, threshold, **kwargs)
    if output_path:
        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return result


# ---- K18: density clusters of regions (DBSCAN) -------------------------------------------------------------

_KIND_NAMES = {2: "core", 1: "border", 0: "noise"}


def density_table(labels, kind, count, border_idx, border_sim, ids, metadatas, *, threshold, min_samples, min_size=1, max_members=None):
    """The JSON-ready report from K18's arrays; a pure function of its arguments (no GPU).

    labels[i] = the cluster of row i (any id, K18 gives the cluster's smallest core row) or -1 for noise, kind[i] = 2 core,
    1 border, 0 noise, count[i] = the row's neighbours, (border_idx, border_sim)[i] = a border row's best core neighbour;
    ids / metadatas are the rows'.  Returns
      {"threshold", "min_samples", "n_regions",
       "clusters": [{"cluster", "size", "n_core", "n_border", "pages": [page names, sorted],
                     "members": [{"id", "parent_image", "box", "kind": "core" | "border", "count",
                                  "best_core": {"id", "score"} (border members only)}, ... in row order]},
                    ... by size descending, then by first member (the lowest row), numbered 0..k-1 in that order],
       "noise": {"count", "ids"},
       "summary": {"n_clusters", "n_core", "n_border", "n_noise", "largest_cluster"}}
    Clusters of fewer than `min_size` rows are left out of "clusters" (they are the tail of the order, so the numbers of the
    others stay; the summary counts all); max_members keeps only the first members of each list (the counts stay whole)."""
    labels, kind, count, border_idx = (np.asarray(v).astype(np.int64).reshape(-1) for v in (labels, kind, count, border_idx))
    border_sim = np.asarray(border_sim, dtype=np.float64).reshape(-1)
    n = len(ids)
    if not (len(labels) == len(kind) == len(count) == len(border_idx) == len(border_sim) == len(metadatas) == n):
        raise ValueError("density_table: labels, kind, count, border_idx, border_sim, ids and metadatas must have one entry per row")
    if n and not np.isin(kind, (0, 1, 2)).all():
        raise ValueError("density_table: kind must be 0 (noise), 1 (border) or 2 (core)")
    if n and ((labels < 0) != (kind == 0)).any():
        raise ValueError("density_table: exactly the noise rows (kind 0) must have the label -1")
    members = {}
    for r in range(n):
        if kind[r] != 0:
            members.setdefault(int(labels[r]), []).append(r)
    order = sorted(members.values(), key=lambda rows: (-len(rows), rows[0]))
    clusters = []
    for number, rows in enumerate(order):
        if len(rows) < max(1, int(min_size)):
            continue
        out_rows = []
        for r in rows:
            m = metadatas[r] or {}
            row = {"id": ids[r], "parent_image": os.path.basename(_parent_of(m)), "box": _box_of(m), "kind": _KIND_NAMES[int(kind[r])],
                   "count": int(count[r])}
            if kind[r] == 1:
                row["best_core"] = {"id": ids[int(border_idx[r])], "score": float(border_sim[r])}
            out_rows.append(row)
        n_core = int(sum(1 for r in rows if kind[r] == 2))
        clusters.append({"cluster": number, "size": len(rows), "n_core": n_core, "n_border": len(rows) - n_core,
                         "pages": sorted({m["parent_image"] for m in out_rows if m["parent_image"]}),
                         "members": out_rows if max_members is None else out_rows[: int(max_members)]})
    noise = [ids[r] for r in range(n) if kind[r] == 0]
    return {"threshold": None if threshold is None else float(threshold), "min_samples": int(min_samples), "n_regions": n, "clusters": clusters,
            "noise": {"count": len(noise), "ids": noise},
            "summary": {"n_clusters": len(order), "n_core": int((kind == 2).sum()), "n_border": int((kind == 1).sum()), "n_noise": len(noise),
                        "largest_cluster": len(order[0]) if order else 0}}


def density_clusters(collection, threshold, min_samples, *, exclude="none", prefix_length=config.PREFIX_LENGTH,
                     where={"is_region": {"$eq": True}}, min_size=1, engine: Engine | None = None):
    """Density clusters (DBSCAN, kernel K18) of the regions `where` selects, rows without an embedding left out: a region is
    core when at least `min_samples` regions, itself included, have a cosine >= `threshold` with it; clusters are the
    connected components of the core regions, a non-core region next to a core one is a border member of its most similar
    core neighbour's cluster, every other region is noise.  Returns density_table's dict.

    `threshold` and `min_samples` have no defaults: the right values belong to the encoder and the archive
    (kth_neighbour_similarity gives the curve to read a threshold from).  exclude: duplicate_inputs' rules for the pairs that
    never count; the default "none" counts every pair -- a page with twelve look-alike columns is density too."""
    if int(min_samples) < 1:
        raise ValueError(f"density_clusters: min_samples = {min_samples}; supported: at least 1")
    all_entries, have = _region_rows(collection, where)
    if not have:
        logger.warning("No regions found in the database. Make sure regions have been processed first.")
        return density_table([], [], [], [], [], [], [], threshold=threshold, min_samples=min_samples, min_size=min_size)
    ids = [all_entries["ids"][r] for r in have]
    metas = [all_entries["metadatas"][r] for r in have]
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)
    group, _, _ = duplicate_inputs(metas, exclude, prefix_length)
    res = engine.density_clusters(emb, float(threshold), int(min_samples), group)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}
    return density_table(host["labels"], host["kind"], host["count"], host["border_idx"], host["border_sim"], ids, metas, threshold=threshold,
                         min_samples=min_samples, min_size=min_size)


def create_density_report(collection, threshold, min_samples, output_path=None, **kwargs):
    """density_clusters, written as one JSON document when `output_path` is given (as create_duplicate_report)."""
    result = density_clusters(collection, threshold, min_samples, **kwargs)
    if output_path:
        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return result


# ---- K19: the cluster hierarchy of regions (mutual-reachability spanning tree) -----------------------------
# Everything below is a pure function of the tree's edge list: no GPU, no further pass over the table.


def _tree_arrays(edges, weights, n=None):
    """(edges int64 [E, 2] as (lo, hi), weights float64 [E], n) sorted by the order of the tree: weight descending, then lo,
    then hi ascending"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(e) != len(w):
        raise ValueError("hierarchy: edges and weights must have one entry per edge")
    e = np.stack([e.min(1), e.max(1)], axis=1) if len(e) else e
    n = (int(e.max()) + 1 if len(e) else 0) if n is None else int(n)
    if len(e) and (e.min() < 0 or e.max() >= n or (e[:, 0] == e[:, 1]).any()):
        raise ValueError(f"hierarchy: edges must join two different rows of 0..{n - 1}")
    order = np.lexsort((e[:, 1], e[:, 0], -w))
    return e[order], w[order], n


def _find(top, x):
    r = x
    while top[r] != r:
        r = top[r]
    while top[x] != r:
        top[x], x = r, top[x]
    return r


def cut_hierarchy(edges, weights, core, threshold):
    """The DBSCAN* clusters at `threshold` from the tree of Engine.hierarchy: (labels, kind), int32 [N].  The rows with core[i]
    >= threshold are core (kind 2); the clusters are the components of the edges with weight >= threshold, which join core rows
    only; a cluster's id is its smallest member; every other row is noise (label -1, kind 0).  These are K18's core rows and
    K18's clusters on them at min_sim = threshold, with K18's border rows as noise."""
    core = np.asarray(core, dtype=np.float64).reshape(-1)
    n = len(core)
    e, w, _ = _tree_arrays(edges, weights, n)
    is_core = core >= threshold
    top = list(range(n))
    for (a, b), keep in zip(e.tolist(), (w >= threshold).tolist()):
        if not keep:
            break  # sorted by weight descending
        ra, rb = _find(top, a), _find(top, b)
        if ra != rb:
            top[max(ra, rb)] = min(ra, rb)  # the root is the smallest member
    labels = np.fromiter((_find(top, r) for r in range(n)), dtype=np.int32, count=n)
    labels = np.where(is_core, labels, -1).astype(np.int32)
    return labels, np.where(is_core, 2, 0).astype(np.int32)


def _single_linkage(e, w, n):
    """The dendrogram of the sorted tree: (left, right, dist, size), one entry per merge, node ids as scipy's (rows 0..n-1, merge
    t is node n + t).  Distance = max(0, 1 - weight); equal weights merge in the order of the tree.  The components of a forest
    are joined at distance +inf, in the order of their smallest members."""
    top = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    left, right, dist = [], [], []
    pairs = e.tolist()
    ds = np.maximum(0.0, 1.0 - w).tolist()
    if len(pairs) > n - 1:
        raise ValueError("hierarchy: the edges close a cycle")

    def merge(a, b, dt):
        node = n + len(left)
        top[a] = top[b] = node
        size[node] = size[a] + size[b]
        left.append(a)
        right.append(b)
        dist.append(dt)
        return node

    for (x, y), dt in zip(pairs, ds):
        a, b = _find(top, x), _find(top, y)
        if a == b:
            raise ValueError("hierarchy: the edges close a cycle")
        merge(a, b, dt)
    if len(pairs) < n - 1:
        roots, seen = [], set()  # in the order of their smallest members
        for r in range(n):
            f = _find(top, r)
            if f not in seen:
                seen.add(f)
                roots.append(f)
        joined = roots[0]
        for f in roots[1:]:
            joined = merge(joined, f, float("inf"))
    return left, right, dist, size


def linkage_of(edges, weights):
    """The tree as a scipy linkage matrix, float64 [N - 1, 4] (node, node, distance = max(0, 1 - weight), rows below), for
    scipy.cluster.hierarchy.dendrogram / fcluster: what the reference draws for pages (weighted_region_clustering.py:297-339),
    for regions.  Needs a spanning tree (N - 1 edges); with min_samples = 1 it is the single-linkage dendrogram of the
    cosine distance."""
    e, w, n = _tree_arrays(edges, weights, None)
    n = max(n, len(e) + 1)
    if len(e) != n - 1:
        raise ValueError(f"linkage_of: {len(e)} edges over {n} rows are a forest, not a tree")
    left, right, dist, size = _single_linkage(e, w, n)
    z = np.empty((n - 1, 4), dtype=np.float64)
    z[:, 0], z[:, 1] = np.minimum(left, right), np.maximum(left, right)
    z[:, 2], z[:, 3] = dist, size[n:]
    return z


def hierarchy_clusters(edges, weights, core, min_cluster_size, *, allow_single_cluster=False):
    """HDBSCAN's threshold-free clusters from the tree of Engine.hierarchy: the condensed tree and the excess-of-mass selection
    as scikit-learn's HDBSCAN does them (cluster_selection_method="eom", no epsilon), with distance = max(0, 1 - weight) and
    lambda = 1 / distance.  Equal-weight merges are processed in the order of the tree (weight descending, lo, hi).  Returns
      {"labels": int32 [N], a cluster's id is its smallest member, -1 for noise,
       "persistence": {cluster id: the cluster's stability, sum over its rows of (lambda_row - lambda_birth)},
       "strength": float64 [N], lambda_row / lambda_max of the row's cluster (1 for a row that never leaves it, 0 for noise)}.
    `core` gives the number of rows (rows without an edge are noise)."""
    n = len(np.asarray(core).reshape(-1))
    mcs = int(min_cluster_size)
    if mcs < 2:
        raise ValueError(f"hierarchy_clusters: min_cluster_size = {min_cluster_size}; supported: at least 2")
    labels = np.full(n, -1, dtype=np.int32)
    strength = np.zeros(n, dtype=np.float64)
    if n < 2:
        return {"labels": labels, "persistence": {}, "strength": strength}
    e, w, _ = _tree_arrays(edges, weights, n)
    left, right, dist, size = _single_linkage(e, w, n)

    def rows_below(node):
        out, stack = [], [node]
        while stack:
            x = stack.pop()
            if x < n:
                out.append(x)
            else:
                stack.append(right[x - n])
                stack.append(left[x - n])
        return out

    # the condensed tree, breadth first, so that a cluster's number is above its parent's: cluster 0 is the root
    c_parent, c_birth = [-1], [0.0]
    own = [[]]       # (row, lambda) of the rows that leave the cluster itself
    children = [[]]  # the two clusters it splits into
    queue = [(2 * n - 2, 0)]
    for node, c in queue:  # grows while it is walked
        while True:
            l, r, d = left[node - n], right[node - n], dist[node - n]
            lam = 1.0 / d if d > 0.0 else float("inf")
            big_l, big_r = size[l] >= mcs, size[r] >= mcs
            if big_l and big_r:
                for side in (l, r):
                    c_parent.append(c)
                    c_birth.append(lam)
                    own.append([])
                    children.append([])
                    children[c].append(len(c_parent) - 1)
                    queue.append((side, len(c_parent) - 1))
                break
            for side, big in ((l, big_l), (r, big_r)):
                if not big:
                    own[c].extend((x, lam) for x in rows_below(side))
            if not big_l and not big_r:
                break
            node = l if big_l else r  # the cluster goes on in its big side
    k = len(c_parent)
    c_size = [0] * k
    for c in range(k - 1, -1, -1):
        c_size[c] += len(own[c])
        if c:
            c_size[c_parent[c]] += c_size[c]

    def excess(lam, birth):
        return 0.0 if lam == birth else lam - birth  # inf - inf: rows that leave at the distance they joined at

    stability = [sum(excess(lam, c_birth[c]) for _, lam in own[c]) + sum(excess(c_birth[ch], c_birth[c]) * c_size[ch] for ch in children[c])
                 for c in range(k)]
    selected = [True] * k
    if not allow_single_cluster:
        selected[0] = False
    for c in range(k - 1, -1 if allow_single_cluster else 0, -1):
        below = sum(stability[ch] for ch in children[c])
        if below > stability[c]:
            selected[c] = False
            stability[c] = below
        else:
            stack = list(children[c])
            while stack:
                x = stack.pop()
                selected[x] = False
                stack.extend(children[x])
    chosen = [c for c in range(k) if selected[c]]
    owner = [-1] * k  # the selected cluster a cluster's rows belong to
    for c in range(k):
        owner[c] = c if selected[c] else (owner[c_parent[c]] if c else -1)
    only_root = chosen == [0]
    # the largest lambda at which a row or a sub-cluster leaves the cluster itself (scikit-learn's lambda_max: a row of a
    # sub-cluster that was not selected has strength 1)
    deaths = [max([lam for _, lam in own[c]] + [c_birth[ch] for ch in children[c]] + [0.0]) for c in range(k)]
    root_threshold = deaths[0]
    members = {}
    for c in range(k):
        o = owner[c]
        if o < 0:
            continue
        for x, lam in own[c]:
            if only_root and lam < root_threshold:
                continue  # scikit-learn: with the root alone selected, a row belongs to it only from the root's last split on
            members.setdefault(o, []).append((x, lam))
    persistence = {}
    for o, rows in members.items():
        ident = min(x for x, _ in rows)
        persistence[int(ident)] = float(stability[o])
        top = deaths[o]
        for x, lam in rows:
            labels[x] = ident
            strength[x] = 1.0 if top == 0.0 or lam == float("inf") else min(lam, top) / top
    return {"labels": labels, "persistence": persistence, "strength": strength}


@dataclasses.dataclass
class RegionHierarchy:
    """The cluster hierarchy of a set of regions (region_hierarchy): the tree's edge list and the rows' ids.  edges int32
    [E, 2] (lo, hi) and weights float32 [E] sorted by weight descending, then lo, then hi; core float32 [N]."""
    edges: np.ndarray
    weights: np.ndarray
    core: np.ndarray
    min_samples: int
    ids: list
    metadatas: list | None = None
    rounds: int = 0
    components: int = 1

    def cut(self, threshold, *, min_size=1, max_members=None):
        """The DBSCAN* clusters at `threshold` as density_table's dict (cut_hierarchy: K18's core rows and clusters at that
        threshold, its border rows among the noise; a member has no "count", which the tree does not hold)."""
        labels, kind = cut_hierarchy(self.edges, self.weights, self.core, threshold)
        n = len(self.ids)
        metas = self.metadatas if self.metadatas is not None else [None] * n
        table = density_table(labels, kind, np.zeros(n, dtype=np.int64), np.full(n, -1), np.zeros(n), self.ids, metas, threshold=threshold,
                              min_samples=self.min_samples, min_size=min_size, max_members=max_members)
        for c in table["clusters"]:
            for m in c["members"]:
                del m["count"]
        return table

    def clusters(self, min_cluster_size, *, allow_single_cluster=False):
        """hierarchy_clusters over the tree, by id: {"min_cluster_size", "n_regions", "clusters": [{"cluster", "size",
        "persistence", "members": [{"id", "strength"}, ... in row order]}, ... by size descending, then first member], "noise":
        {"count", "ids"}, "labels": int32 [N] (a cluster's smallest row, -1 noise)}."""
        res = hierarchy_clusters(self.edges, self.weights, self.core, min_cluster_size, allow_single_cluster=allow_single_cluster)
        members = {}
        for r, lab in enumerate(res["labels"].tolist()):
            if lab >= 0:
                members.setdefault(lab, []).append(r)
        out = []
        for number, (lab, rows) in enumerate(sorted(members.items(), key=lambda kv: (-len(kv[1]), kv[0]))):
            out.append({"cluster": number, "size": len(rows), "persistence": res["persistence"][lab],
                        "members": [{"id": self.ids[r], "strength": float(res["strength"][r])} for r in rows]})
        noise = [self.ids[r] for r in np.flatnonzero(res["labels"] < 0).tolist()]
        return {"min_cluster_size": int(min_cluster_size), "n_regions": len(self.ids), "clusters": out,
                "noise": {"count": len(noise), "ids": noise}, "labels": res["labels"]}

    def linkage(self):
        """linkage_of over the tree: the scipy linkage matrix of the regions' dendrogram (label its leaves with `ids`)."""
        return linkage_of(self.edges, self.weights)


def region_hierarchy(collection, min_samples, *, exclude="none", prefix_length=config.PREFIX_LENGTH, where={"is_region": {"$eq": True}},
                     engine: Engine | None = None):
    """The cluster hierarchy (kernel K19, Engine.hierarchy) of the regions `where` selects, rows without an embedding left out:
    the spanning tree of the mutual-reachability graph, computed once on the GPU.  -> RegionHierarchy, whose .cut(threshold)
    gives the DBSCAN* clusters at ANY threshold, .clusters(min_cluster_size) HDBSCAN's threshold-free ones and .linkage() the
    dendrogram, all on the host.

    `min_samples` has no default: the right value belongs to the archive.  exclude: duplicate_inputs' rules for the pairs that
    never count, as density_clusters."""
    if int(min_samples) < 1:
        raise ValueError(f"region_hierarchy: min_samples = {min_samples}; supported: at least 1")
    all_entries, have = _region_rows(collection, where)
    if not have:
        logger.warning("No regions found in the database. Make sure regions have been processed first.")
        return RegionHierarchy(np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32), int(min_samples), [], [],
                               0, 0)
    ids = [all_entries["ids"][r] for r in have]
    metas = [all_entries["metadatas"][r] for r in have]
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)
    group, _, _ = duplicate_inputs(metas, exclude, prefix_length)
    res = engine.hierarchy(emb, int(min_samples), group)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}
    return RegionHierarchy(host["edges"].astype(np.int32), host["weights"].astype(np.float32), host["core"].astype(np.float32), int(min_samples), ids,
                           metas, int(res["rounds"]), int(res["components"]))


def create_hierarchy_report(collection, min_samples, output_path=None, *, thresholds=(), min_cluster_size=None, **kwargs):
    """region_hierarchy, written as one JSON document when `output_path` is given (as create_density_report): the tree by id
    ({"a", "b", "weight"} per edge, in the tree's order), every row's core similarity, the cut at each of `thresholds` and,
    with `min_cluster_size`, the threshold-free clusters."""
    h = region_hierarchy(collection, min_samples, **kwargs)
    result = {"min_samples": int(min_samples), "n_regions": len(h.ids), "rounds": h.rounds, "components": h.components,
              "edges": [{"a": h.ids[a], "b": h.ids[b], "weight": float(w)} for (a, b), w in zip(h.edges.tolist(), h.weights.tolist())],
              "core": {i: float(c) for i, c in zip(h.ids, h.core.tolist())},
              "cuts": [h.cut(t) for t in thresholds]}
    if min_cluster_size is not None:
        clusters = h.clusters(min_cluster_size)
        clusters["labels"] = clusters["labels"].tolist()
        result["clusters"] = clusters
    if output_path:
        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return result


K12_LIST_LIMIT = 128  # mme_neighbours: fetch and top_n lie in 1..128


def kth_neighbour_similarity(collection, k, *, exclude="none", where={"is_region": {"$eq": True}}, engine: Engine | None = None):
    """The cosine of every region's k-th most similar admissible region, as a float32 array sorted descending: the curve whose
    knee is the usual way to choose density_clusters' threshold for min_samples = k + 1.  One pass of K12 (Engine.neighbours)
    over the rows `where` selects, rows without an embedding left out; exclude: duplicate_inputs' rules.  A row with fewer than
    k admissible rows has no such value and is left out.

    K12's lists hold at most `fetch` = 128 rows, the row itself and the rows `exclude` drops among them.  ValueError names the
    limit when k does not fit (k <= 127 under "none", k <= 128 otherwise), or when a row's 128 nearest rows hold fewer than k
    admissible ones although the table has them."""
    k = int(k)
    if exclude not in ("parent", "prefix", "none"):
        raise ValueError("exclude must be 'parent', 'prefix' or 'none'")
    most = K12_LIST_LIMIT - 1 if exclude == "none" else K12_LIST_LIMIT
    if k < 1 or k > most:
        raise ValueError(f"kth_neighbour_similarity: k = {k}; supported 1..{most} under exclude = {exclude!r} (K12's lists hold fetch <= "
                         f"{K12_LIST_LIMIT} rows, the row itself among them, and top_n <= {K12_LIST_LIMIT})")
    all_entries, have = _region_rows(collection, where)
    if not have:
        return np.empty(0, dtype=np.float32)
    metas = [all_entries["metadatas"][r] for r in have]
    n = len(have)
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)
    group, _, _ = duplicate_inputs(metas, exclude)
    fetch = min(k + 1, K12_LIST_LIMIT) if group is None else K12_LIST_LIMIT
    idx, sim = engine.neighbours(emb, group, fetch=fetch, top_n=k)
    idx = idx.cpu().numpy() if hasattr(idx, "cpu") else np.asarray(idx)
    sim = sim.cpu().numpy() if hasattr(sim, "cpu") else np.asarray(sim)
    found = idx[:, k - 1] >= 0
    if group is None:
        admissible = np.full(n, n - 1)
    else:
        _, inverse, size = np.unique(group, return_inverse=True, return_counts=True)
        admissible = n - size[inverse]
    short = ~found & (admissible >= k)
    if short.any():
        raise ValueError(f"kth_neighbour_similarity: {int(short.sum())} rows have fewer than k = {k} admissible rows among their fetch = "
                         f"{K12_LIST_LIMIT} nearest (K12's limit on the list length) under exclude = {exclude!r}")
    return np.sort(sim[found, k - 1].astype(np.float32))[::-1].copy()


# ---- K15: k groups of look-alike regions (spherical k-means) ---------------------------------------------

def cluster_table(labels, sim, ids, metadatas, *, n_clusters=None, iterations=None, converged=None, objective=None, max_members=None):
    """The JSON-ready report from K15's arrays; a pure function of its arguments (no GPU).

    labels[i] = the cluster of row i, sim[i] = its cosine to that cluster's centroid; ids / metadatas are the rows'.  Returns
      {"n_regions", "n_clusters", "n_empty", "iterations", "converged", "objective",
       "clusters": [{"cluster", "size", "cohesion": mean sim or None, "medoid": id of the member with the largest sim (the lowest
                     row among equals) or None, "pages": [page names, sorted],
                     "members": [{"id", "parent_image", "type", "area_percentage", "score"}, ... by score descending, then row]},
                    ... cluster 0 .. n_clusters - 1; an empty cluster is listed with size 0, never renumbered]}
    n_clusters defaults to max(labels) + 1; max_members keeps only the best members of each list (size and cohesion stay whole)."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    sim = np.asarray(sim, dtype=np.float64).reshape(-1)
    n = len(ids)
    if not (len(labels) == len(sim) == len(metadatas) == n):
        raise ValueError("cluster_table: labels, sim, ids and metadatas must have one entry per row")
    k = (int(labels.max()) + 1 if n else 0) if n_clusters is None else int(n_clusters)
    if n and (labels.min() < 0 or labels.max() >= k):
        raise ValueError(f"cluster_table: labels must lie in 0..{k - 1}")
    members = [[] for _ in range(k)]
    for r in range(n):
        members[int(labels[r])].append(r)
    clusters = []
    for j, rows in enumerate(members):
        rows = sorted(rows, key=lambda r: (-sim[r], r))  # a NaN score would not sort: K15 gives none on unit rows
        out_rows = []
        for r in rows:
            m = metadatas[r] or {}
            out_rows.append({"id": ids[r], "parent_image": os.path.basename(_parent_of(m)), "type": m.get("region_type", "unknown"),
                             "area_percentage": m.get("area_percentage", 0), "score": float(sim[r])})
        clusters.append({"cluster": j, "size": len(rows), "cohesion": float(np.mean(sim[rows])) if rows else None,
                         "medoid": ids[rows[0]] if rows else None,
                         "pages": sorted({m["parent_image"] for m in out_rows if m["parent_image"]}),
                         "members": out_rows if max_members is None else out_rows[: int(max_members)]})
    return {"n_regions": n, "n_clusters": k, "n_empty": sum(1 for c in clusters if c["size"] == 0),
            "iterations": None if iterations is None else int(iterations), "converged": None if converged is None else bool(converged),
            "objective": None if objective is None else float(objective), "clusters": clusters}


def kmeans_init_rows(emb, k, init="k-means++", seed=0):
    """k distinct start rows of the unit rows emb [N, d] (a torch tensor on any device), sorted, as int32 numpy.

    init = "k-means++": the first row uniform, each further row with probability proportional to 1 - (its largest cosine to the
    rows chosen so far), from a torch.Generator on emb's device seeded with `seed` (plain torch: k matrix-vector products);
    "random": numpy.random.default_rng(seed).choice without replacement; an int array: those rows (checked, not sorted)."""
    import torch

    n, k = int(emb.shape[0]), int(k)
    if k < 1 or k > n:
        raise ValueError(f"n_clusters = {k} must lie in 1..{n} (the number of rows)")
    if not isinstance(init, str):
        rows = np.asarray(init)
        if rows.ndim != 1 or rows.size != k or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError(f"init rows must be a 1-D integer array of n_clusters = {k} rows")
        if rows.min() < 0 or rows.max() >= n:
            raise ValueError(f"init rows must lie in 0..{n - 1}")
        if len(np.unique(rows)) != k:
            raise ValueError("init rows must be distinct")
        return rows.astype(np.int32)
    if init == "random":
        return np.sort(np.random.default_rng(int(seed)).choice(n, size=k, replace=False)).astype(np.int32)
    if init != "k-means++":
        raise ValueError("init must be 'k-means++', 'random' or an integer array of rows")
    g = torch.Generator(device=emb.device).manual_seed(int(seed))
    x = emb.to(torch.float32)
    chosen = torch.zeros(n, dtype=torch.bool, device=emb.device)
    first = int(torch.randint(0, n, (1,), generator=g, device=emb.device).item())
    rows = [first]
    chosen[first] = True
    dist = (1.0 - x @ x[first]).clamp_(min=0.0)
    for _ in range(1, k):
        w = dist.masked_fill(chosen, 0.0)
        if float(w.sum().item()) <= 0.0:  # every row left is a copy of a chosen one: take the lowest
            nxt = int(torch.nonzero(~chosen)[0].item())
        else:
            nxt = int(torch.multinomial(w, 1, generator=g).item())
        rows.append(nxt)
        chosen[nxt] = True
        dist = torch.minimum(dist, (1.0 - x @ x[nxt]).clamp_(min=0.0))
    return np.sort(np.asarray(rows)).astype(np.int32)


def _region_rows(collection, where):
    all_entries = collection.get(include=["metadatas", "embeddings", "documents"], where=where)
    have = [r for r, e in enumerate((all_entries or {}).get("embeddings") or []) if e is not None and len(e) > 0]
    return all_entries, have


def pick_n_clusters(scores):
    """The number of clusters from {k: silhouette score or None}: the page side's rule (oracle/cluster.py, cluster_images).  k
    ascending, the best score starting at -1 and the answer at the first k; a k is taken only when its score is strictly
    above the best so far, and a k without a score (None or NaN) is skipped.  Pure: no GPU."""
    ks = sorted(int(k) for k in scores)
    if not ks:
        raise ValueError("pick_n_clusters: no k to choose from")
    best_score, best_k = -1, ks[0]
    by_int = {int(k): v for k, v in scores.items()}
    for k in ks:
        v = by_int[k]
        if v is None or v != v:
            continue
        if v > best_score:
            best_score, best_k = v, k
    return best_k


def _clip_k_range(k_range, n):
    ks = sorted({int(k) for k in k_range if 2 <= int(k) <= n})
    if not ks:
        raise ValueError(f"k_range holds no k in 2..{n} (the number of regions)")
    return ks


def _score_or_none(v):
    v = float(v)
    return None if v != v else v


def cluster_regions(collection, n_clusters, *, where={"is_region": {"$eq": True}}, init="k-means++", seed=0, n_init=1, max_iter=100,
                    engine: Engine | None = None, max_members=None, k_range=range(2, 11), silhouette=False):
    """n_clusters groups of look-alike regions: spherical k-means (kernel K15) over the unit bf16 vectors of the rows `where`
    selects (rows without an embedding left out).  Returns cluster_table's dict; kmeans_regions also returns the arrays
    (the centroids among them, which assign_regions takes).

    init: kmeans_init_rows' forms; run r of n_init uses seed + r, and the run with the largest objective (the sum of the
    rows' cosines to their centroids) is kept, the first among equals.

    n_clusters = None (given explicitly: the argument keeps no default) chooses it: every k of k_range (clipped to 2..the number of regions) gets such a run and one silhouette
    (kernel K16) of the run kept; pick_n_clusters decides, and the table of that k comes back with "k_scores" ({k: score or
    None}), "silhouette" (the picked k's score) and a "silhouette" entry in each cluster (its mean, None for an empty one).
    With a given n_clusters those keys appear only under silhouette=True."""
    table, _ = kmeans_regions(collection, n_clusters, where=where, init=init, seed=seed, n_init=n_init, max_iter=max_iter, engine=engine,
                              max_members=max_members, k_range=k_range, silhouette=silhouette)
    return table


def kmeans_regions(collection, n_clusters, *, where={"is_region": {"$eq": True}}, init="k-means++", seed=0, n_init=1, max_iter=100,
                   engine: Engine | None = None, max_members=None, k_range=range(2, 11), silhouette=False, silhouette_samples=False):
    """cluster_regions, returning (table, arrays): arrays = {"ids", "labels", "sim", "centroids" (bf16 CUDA tensor), "counts",
    "objectives" (one per run), "best_run"} or None without regions; with n_clusters = None also "by_k" ({k: {"labels",
    "objectives", "best_run", "silhouette"}}), and under silhouette_samples=True "silhouette_samples" (float64 [n])."""
    if int(n_init) < 1:
        raise ValueError(f"n_init = {n_init} must be at least 1")
    if int(max_iter) < 0 or int(max_iter) > 1000:
        raise ValueError(f"max_iter = {max_iter} must lie in 0..1000")
    all_entries, have = _region_rows(collection, where)
    if not have:
        logger.warning("No regions found in the database. Make sure regions have been processed first.")
        return cluster_table([], [], [], [], n_clusters=0), None
    ids = [all_entries["ids"][r] for r in have]
    metas = [all_entries["metadatas"][r] for r in have]
    choose = n_clusters is None
    if choose:
        ks = _clip_k_range(k_range, len(ids))
    else:
        if int(n_clusters) < 1 or int(n_clusters) > len(ids):
            raise ValueError(f"n_clusters = {n_clusters} must lie in 1..{len(ids)} (the number of regions)")
        ks = [int(n_clusters)]
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)  # one upload for every k
    want_sil = choose or bool(silhouette) or bool(silhouette_samples)
    runs = {}
    for k in ks:
        best, objectives, best_run = None, [], 0
        for run in range(int(n_init)):
            rows = kmeans_init_rows(emb, k, init, int(seed) + run)
            res = engine.kmeans(emb, k, init_rows=rows, max_iter=int(max_iter))
            obj = float(res.objective.item())
            objectives.append(obj)
            if best is None or obj > objectives[best_run]:
                best, best_run = res, run
        sil = engine.silhouette(emb, best.labels, k, samples=bool(silhouette_samples)) if want_sil else None
        runs[k] = (best, objectives, best_run, sil)
    k_scores = {k: _score_or_none(r[3].score.item()) for k, r in runs.items()} if want_sil else None
    k = pick_n_clusters(k_scores) if choose else ks[0]
    best, objectives, best_run, sil = runs[k]
    info = best.info.cpu().numpy()
    labels, sim = best.labels.cpu().numpy(), best.sim.cpu().numpy()
    table = cluster_table(labels, sim, ids, metas, n_clusters=k, iterations=int(info[0]), converged=bool(info[2]),
                          objective=objectives[best_run], max_members=max_members)
    arrays = {"ids": ids, "labels": labels, "sim": sim, "centroids": best.centroids, "counts": best.counts.cpu().numpy(),
              "objectives": objectives, "best_run": best_run}
    if want_sil:
        table["k_scores"] = k_scores
        table["silhouette"] = k_scores[k]
        for c, v in zip(table["clusters"], sil.cluster.cpu().numpy()):
            c["silhouette"] = _score_or_none(v)
        if silhouette_samples:
            arrays["silhouette_samples"] = sil.samples.cpu().numpy()
    if choose:
        arrays["by_k"] = {kk: {"labels": r[0].labels.cpu().numpy(), "objectives": r[1], "best_run": r[2], "silhouette": k_scores[kk]}
                          for kk, r in runs.items()}
    return table, arrays


def silhouette_regions(collection, labels, *, where={"is_region": {"$eq": True}}, engine: Engine | None = None):
    """The silhouette (kernel K16) of labels the caller already has -- assign_regions' output, say -- one per row `where` selects
    (rows without an embedding left out), in the collection's order; a negative label belongs to no cluster.  Returns
    {"n_regions", "n_clusters", "silhouette", "clusters": [{"cluster", "size", "silhouette": mean or None}], "samples": [per
    row, None for a row of no cluster]}.  ValueError when fewer than two clusters have members."""
    all_entries, have = _region_rows(collection, where)
    labels = np.asarray(labels).reshape(-1)
    if len(labels) != len(have):
        raise ValueError(f"silhouette_regions: {len(labels)} labels for {len(have)} regions")
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("silhouette_regions: labels must be integers")
    n = len(have)
    k = max(int(labels.max()) + 1 if n else 0, 2)
    members = len(np.unique(labels[labels >= 0]))
    if members < 2 or n < 2:
        raise ValueError(f"silhouette_regions: {members} cluster(s) have members; a silhouette needs at least two")
    engine = engine or default_engine()
    emb = to_unit_bf16([all_entries["embeddings"][r] for r in have], engine)
    lab = engine.torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(emb.device)
    res = engine.silhouette(emb, lab, k, samples=True)
    if int(res.info[1].item()) < 2:
        raise ValueError(f"silhouette_regions: {int(res.info[1].item())} cluster(s) have members; a silhouette needs at least two")
    counts = res.counts.cpu().numpy()
    return {"n_regions": n, "n_clusters": k, "silhouette": _score_or_none(res.score.item()),
            "clusters": [{"cluster": j, "size": int(counts[j]), "silhouette": _score_or_none(v)} for j, v in enumerate(res.cluster.cpu().numpy())],
            "samples": [_score_or_none(v) for v in res.samples.cpu().numpy()]}


def assign_regions(centroids, embeddings, *, engine: Engine | None = None):
    """Which existing cluster does each new vector belong to: (labels int32 [n], sim float32 [n]) numpy arrays, the cluster whose
    centroid (bf16 [k, d] tensor, as kmeans_regions returns) has the largest cosine with the row and that cosine.  K15 with
    max_iter = 0: the centroids are not changed.  mme_kmeans wants at least k rows, so fewer are padded with copies of the
    first row, whose results are dropped."""
    engine = engine or default_engine()
    emb = to_unit_bf16(embeddings, engine)
    n, k = int(emb.shape[0]), int(centroids.shape[0])
    if n == 0:
        return np.empty(0, dtype=np.int32), np.empty(0, dtype=np.float32)
    if n < k:
        emb = engine.torch.cat([emb, emb[:1].expand(k - n, -1)]).contiguous()
    res = engine.kmeans(emb, k, centroids=centroids, max_iter=0)
    return res.labels[:n].cpu().numpy(), res.sim[:n].cpu().numpy()


def create_region_cluster_report(collection, n_clusters, output_path=None, **kwargs):
    """cluster_regions (its keywords passed through: n_clusters = None chooses k over k_range by silhouette), written as one
    JSON document when `output_path` is given (as create_duplicate_report)."""
    result = cluster_regions(collection, n_clusters, **kwargs)
    if output_path:
        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            json.dump(result, fh, indent=1)
    return result


# ---- K17: centre, reduce and whiten the vector table -----------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Projection:
    """A mean and a PCA basis fitted on a vector table (fit_projection / projection_from_moments), float64 numpy arrays:
    mean [d]; components [m, d], the rows W_j that `transform` applies (v_j, or v_j / sqrt(lambda_j + eps) when whitened);
    eigenvalues [d], all of them, descending; explained_variance_ratio [d] (each eigenvalue's share of their sum, a negative
    rounding residue counted as 0); n_rows the rows fitted on; whiten, eps as given."""
    mean: np.ndarray
    components: np.ndarray
    eigenvalues: np.ndarray
    explained_variance_ratio: np.ndarray
    n_rows: int
    whiten: bool
    eps: float

    @property
    def n_components(self) -> int:
        return int(self.components.shape[0])

    def transform(self, vectors, *, normalise=True, engine: Engine | None = None):
        """W . (x - mean) of every row of `vectors` (lists of floats, numpy or CUDA tensors [N, d]; rounded to unit bf16 rows the
        way the collection's vectors are; an image vector and a text query vector alike), kernel K17b in f32.  normalise=True:
        the L2-normalised bf16 CUDA rows [N, m] that K9..K16 take (n_components % 64 == 0); normalise=False: the float32 CUDA
        coordinates [N, m] for any m (2 for a map)."""
        m = self.n_components
        if normalise and m % 64 != 0:
            raise ValueError(f"transform: n_components = {m} with normalise=True; supported: a multiple of 64 (normalise=False returns "
                             "float32 coordinates for any n_components)")
        engine = engine or default_engine()
        rows = to_unit_bf16(vectors, engine)
        if rows.shape[1] != self.mean.shape[0]:
            raise ValueError(f"transform: vectors have d = {rows.shape[1]}; supported: d = {self.mean.shape[0]} (what the projection was fitted on)")
        return engine.project(rows, self.mean, self.components, normalise=bool(normalise))


def projection_from_moments(sum, gram, n, n_components, *, whiten=False, eps=0.0, rank_tol=1e-10) -> Projection:
    """The host half of the fit, float64 numpy, no device: from sum [d] = the column sums and gram [d, d] = X^T X of n rows
    (Engine.moments) the mean mu = sum / n, the covariance C = gram / n - mu mu^T (symmetrised), its eigenpairs by
    numpy.linalg.eigh in descending order, every eigenvector signed so that its entry of largest magnitude (the lowest index
    among equals) is positive, and the first n_components of them as rows -- divided by sqrt(lambda_j + eps) under whiten.
    ValueError with the field, the value and the supported set: n < 2, n_components outside 1..d or beyond the numerical rank
    (the number of lambda_j > rank_tol * lambda_0)."""
    s = np.asarray(sum, dtype=np.float64).reshape(-1)
    G = np.asarray(gram, dtype=np.float64)
    d = s.shape[0]
    if G.shape != (d, d):
        raise ValueError(f"projection_from_moments: gram has shape {G.shape}; supported: [d, d] = [{d}, {d}] (sum has {d} columns)")
    n = int(n)
    if n < 2:
        raise ValueError(f"projection_from_moments: n = {n}; supported: at least 2 rows")
    m = int(n_components)
    if m < 1 or m > d:
        raise ValueError(f"projection_from_moments: n_components = {m}; supported 1..d (d = {d})")
    if not float(eps) >= 0.0:
        raise ValueError(f"projection_from_moments: eps = {eps}; supported: eps >= 0")
    mu = s / n
    C = G / n - np.outer(mu, mu)
    C = (C + C.T) / 2
    lam, V = np.linalg.eigh(C)
    lam, V = lam[::-1].copy(), V[:, ::-1].T.copy()  # descending; rows are eigenvectors
    big = np.argmax(np.abs(V), axis=1)  # the first among equals
    V *= np.where(V[np.arange(d), big] < 0, -1.0, 1.0)[:, None]
    rank = int(np.count_nonzero(lam > float(rank_tol) * lam[0])) if lam[0] > 0 else 0
    if m > rank:
        raise ValueError(f"projection_from_moments: n_components = {m}; supported 1..{rank} (the numerical rank of the covariance of {n} rows: "
                         f"eigenvalues above rank_tol = {rank_tol} times the largest)")
    W = V[:m] / np.sqrt(lam[:m] + float(eps))[:, None] if whiten else V[:m].copy()
    pos = np.maximum(lam, 0.0)
    return Projection(mean=mu, components=np.ascontiguousarray(W), eigenvalues=lam, explained_variance_ratio=pos / pos.sum(), n_rows=n,
                      whiten=bool(whiten), eps=float(eps))


def fit_projection(source, n_components, *, whiten=False, eps=0.0, rank_tol=1e-10, where={"is_region": {"$eq": True}},
                   engine: Engine | None = None) -> Projection:
    """A Projection fitted on `source`: a RegionCollection (the rows `where` selects, rows without an embedding left out) or an
    array / tensor [N, d].  The vectors become unit bf16 rows as everywhere (to_unit_bf16), kernel K17a computes their column
    sums and second moments in float64 in a fixed order, and projection_from_moments does the rest on the host.  Exact and
    reproducible: the same table gives the same Projection bit for bit."""
    engine = engine or default_engine()
    if hasattr(source, "get") and hasattr(source, "upsert"):
        all_entries, have = _region_rows(source, where)
        if len(have) < 2:
            raise ValueError(f"fit_projection: N = {len(have)} regions with an embedding; supported: at least 2 rows")
        source = [all_entries["embeddings"][r] for r in have]
    rows = to_unit_bf16(source, engine)
    if rows.shape[0] < 2:
        raise ValueError(f"fit_projection: N = {rows.shape[0]}; supported: at least 2 rows")
    s, g = engine.moments(rows)
    return projection_from_moments(s.cpu().numpy(), g.cpu().numpy(), rows.shape[0], n_components, whiten=whiten, eps=eps, rank_tol=rank_tol)


def project_collection(collection, projection: Projection, engine: Engine | None = None, *, transform=None):
    """A new RegionCollection with the same ids, documents and metadatas in the same order and the projected, L2-normalised
    vectors (Projection.transform; a row without an embedding stays without one).  Its collection-level metadata gains
    {"projection": {"n_components", "whiten", "n_rows"}}.  The source is not changed.  `transform`: what turns the list of
    vectors into the projected rows (array-like [n, m]) in place of projection.transform -- a device-free stand-in."""
    from .weighted_region_clustering import RegionCollection

    rows = collection.get(include=["metadatas", "embeddings", "documents"])
    emb = list(rows.get("embeddings") if rows.get("embeddings") is not None else [])
    have = [r for r, e in enumerate(emb) if e is not None and len(e) > 0]
    out = [None] * len(rows["ids"])
    if have:
        vecs = [emb[r] for r in have]
        y = transform(vecs) if transform is not None else projection.transform(vecs, normalise=True, engine=engine or getattr(collection, "engine", None))
        y = y.float().cpu().numpy() if hasattr(y, "cpu") else np.asarray(y, dtype=np.float32)
        for r, v in zip(have, y):
            out[r] = v
    new = RegionCollection(metric=getattr(collection, "metric", "cosine"), engine=engine or getattr(collection, "engine", None))
    new.metadata = {**getattr(collection, "metadata", {}), "projection": {"n_components": projection.n_components, "whiten": bool(projection.whiten),
                                                                         "n_rows": int(projection.n_rows)}}
    new.upsert(ids=list(rows["ids"]), embeddings=out, documents=list(rows.get("documents") or [None] * len(rows["ids"])),
               metadatas=list(rows["metadatas"]))
    return new
