"""Near-duplicate groups without a GPU: the float64 reference on a hand-drawn graph, the report table, and the conditions
the GPU cases rely on (tests/duplicates_reference.py), so that they are known to hold before anything reaches a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duplicates_reference as R  # noqa: E402

from multimodal_embeddings_amd import region_compare as rc  # noqa: E402


def _hand_drawn():
    """8 rows in d = 64 whose pair similarities are set through a Gram matrix: two triangles {0, 2, 5} and {1, 3, 4} joined by
    the edge 3-5, row 6 isolated, and the pair 6-7 similar but of one group.  Returns (rows, groups)."""
    n = 8
    G = np.eye(n)
    for i, j in [(0, 2), (0, 5), (2, 5), (1, 3), (1, 4), (3, 4), (3, 5)]:
        G[i, j] = G[j, i] = 0.4
    G[5, 2] = G[2, 5] = 0.45   # row 2 and row 5 prefer each other
    G[6, 7] = G[7, 6] = 0.5
    w, V = np.linalg.eigh(G)
    assert w.min() > 0
    x = np.zeros((n, 64))
    x[:, :n] = V * np.sqrt(w)  # rows with x x^T = G
    group = np.array([0, 1, 2, 3, 4, 5, 9, 9], dtype=np.int32)
    return R.to_bf16(x)[0], group


def test_reference_on_a_hand_drawn_graph():
    x32, group = _hand_drawn()
    page = np.array([0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int32)
    tau = 0.3
    ref = R.reference(x32, tau, group, page, 4)
    assert R.dead_zone_pairs(ref["S"], ref["adm"], tau, R.delta(64)) == 0
    assert ref["edges"].tolist() == [[0, 2], [0, 5], [1, 3], [1, 4], [2, 5], [3, 4], [3, 5]]
    assert ref["labels"].tolist() == [0, 0, 0, 0, 0, 0, 6, 7]  # the excluded pair 6-7 stays apart
    assert ref["degree"].tolist() == [2, 2, 2, 3, 2, 3, 0, 0]
    assert ref["best_idx"].tolist()[2] == 5 and ref["best_idx"].tolist()[5] == 2 and ref["best_idx"].tolist()[6:] == [-1, -1]
    assert ref["best_sim"][6] == 0 and abs(ref["best_sim"][2] - 0.45) < 0.01
    assert ref["summary"].tolist() == [7, 1, 6, 6]
    # pages: 0-2 -> (0,1); 0-5 -> (0,2); 1-3 -> (0,1); 1-4 -> (0,2); 2-5 -> (1,2); 3-4 -> (1,2); 3-5 -> (1,2)
    assert ref["page_pairs"].tolist() == [[0, 2, 2, 0], [2, 0, 3, 0], [2, 3, 0, 0], [0, 0, 0, 0]]
    # without groups the pair 6-7 is an edge, and within-page edges land on the diagonal
    free = R.reference(x32, tau, None, page, 4)
    assert free["labels"].tolist() == [0, 0, 0, 0, 0, 0, 6, 6] and free["summary"].tolist() == [8, 2, 8, 6]
    assert free["page_pairs"][3, 3] == 1 and np.array_equal(free["page_pairs"], free["page_pairs"].T)
    # a tie goes to the lower index: rows 0 and 1 doubled
    t32 = np.concatenate([x32[:1], x32[:1], x32[:1]])
    tie = R.reference(t32, 0.5)
    assert tie["best_idx"].tolist() == [1, 0, 0] and tie["labels"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("n,d", R.SHAPES)
def test_generator_leaves_the_dead_zone_empty(n, d):
    """gap >= 2 delta is what the contract needs; the cases keep 4 delta"""
    for seed in (1, 2, 3):
        x32, _ = R.walks(n, d, seed)
        S = R.similarity(x32)
        tau, gap = R.widest_gap(S)
        assert R.WINDOW[0] < tau < R.WINDOW[1] and gap >= 4 * R.delta(d), (seed, gap / R.delta(d))
        assert R.dead_zone_pairs(S, R.admissible(n), tau, R.delta(d)) == 0
    c = R.case(n, d, 1)
    sizes = np.bincount(c["ref"]["labels"], minlength=n)
    assert c["dead"] == 0 and 70 <= len(c["ref"]["edges"]) <= 600 and sizes.max() >= 5 and (sizes == 1).sum() >= 10
    assert c["ref"]["ambiguous"].sum() <= 0.01 * n
    if (n, d) in ((331, 128), (515, 768)):
        g = R.case(n, d, 1, 12)
        assert g["dead"] == 0 and 0 < len(g["ref"]["edges"]) < len(c["ref"]["edges"]) and np.trace(g["ref"]["page_pairs"]) == 0
        assert g["ref"]["page_pairs"].sum() == 2 * len(g["ref"]["edges"])


def _rows():
    ids = [f"r{i}" for i in range(8)]
    metas = [{"parent_image": f"/p/page{i // 2}.png", "region_type": "advert" if i % 2 else "text", "area_percentage": 1.5 * i} for i in range(8)]
    metas[7] = None
    return ids, metas


def test_group_table_orders_groups_and_members():
    ids, metas = _rows()
    labels = [0, 1, 1, 0, 4, 1, 6, 4]
    degree = [1, 2, 1, 1, 1, 1, 0, 1]
    best_idx = [3, 2, 1, 0, 7, 1, -1, 4]
    best_sim = [0.9, 0.8, 0.8, 0.9, 0.7, 0.75, 0.0, 0.7]
    t = rc.group_table(labels, degree, best_idx, best_sim, ids, metas, threshold=0.6)
    assert t["threshold"] == 0.6 and t["n_regions"] == 8 and t["n_edges"] == 4 and "edges" not in t and "page_overlap" not in t
    # size descending, then first member
    assert [(g["size"], g["members"][0]["id"]) for g in t["groups"]] == [(3, "r1"), (2, "r0"), (2, "r4")]
    g = t["groups"][0]
    assert [m["id"] for m in g["members"]] == ["r1", "r2", "r5"] and g["pages"] == ["page0.png", "page1.png", "page2.png"]
    assert g["members"][0] == {"id": "r1", "parent_image": "page0.png", "type": "advert", "area_percentage": 1.5, "degree": 2,
                               "best_match": {"id": "r2", "score": 0.8}}
    # a row without metadata is still a member, with the placeholders region_neighbours uses
    last = t["groups"][2]["members"][1]
    assert last["id"] == "r7" and last["parent_image"] == "" and last["type"] == "unknown" and t["groups"][2]["pages"] == ["page2.png"]
    # min_size: 1 lists the singleton too (no best match), 3 keeps the one large group
    one = rc.group_table(labels, degree, best_idx, best_sim, ids, metas, min_size=1)
    assert [g["size"] for g in one["groups"]] == [3, 2, 2, 1] and one["groups"][3]["members"][0]["best_match"] is None
    assert one["threshold"] is None
    assert [g["size"] for g in rc.group_table(labels, degree, best_idx, best_sim, ids, metas, min_size=3)["groups"]] == [3]
    with pytest.raises(ValueError):
        rc.group_table(labels[:-1], degree, best_idx, best_sim, ids, metas)


def test_group_table_edges_and_page_overlap():
    ids, metas = _rows()
    labels, degree = [0, 1, 1, 0, 4, 1, 6, 4], [1, 2, 1, 1, 1, 1, 0, 1]
    best_idx, best_sim = [3, 2, 1, 0, 7, 1, -1, 4], [0.9, 0.8, 0.8, 0.9, 0.7, 0.75, 0.0, 0.7]
    edges = np.array([[4, 7], [1, 5], [0, 3], [1, 2]], dtype=np.int32)
    sims = np.array([0.7, 0.75, 0.9, 0.8], dtype=np.float32)
    pp = np.arange(16, dtype=np.int32).reshape(4, 4)
    names = ["page0.png", "page1.png", "page2.png", "page3.png"]
    t = rc.group_table(labels, degree, best_idx, best_sim, ids, metas, page_pairs=pp, image_names=names, edges=edges, edge_sim=sims, n_edges=4)
    assert t["page_overlap"] == {"image_names": names, "counts": pp.tolist()}
    assert [(e["a"], e["b"]) for e in t["edges"]["pairs"]] == [("r0", "r3"), ("r1", "r2"), ("r1", "r5"), ("r4", "r7")]
    assert t["edges"]["pairs"][0]["score"] == pytest.approx(0.9) and t["edges"]["truncated"] is False
    cut = rc.group_table(labels, degree, best_idx, best_sim, ids, metas, edges=edges[:2], edge_sim=sims[:2], n_edges=4)
    assert cut["edges"]["truncated"] is True and len(cut["edges"]["pairs"]) == 2 and cut["n_edges"] == 4
    import json

    assert json.loads(json.dumps(t)) == t  # JSON-ready: no numpy scalars


def test_duplicate_inputs_by_parent_prefix_and_none():
    metas = [{"parent_image": "/a/issue1_p1.png"}, {"parent_image_name": "issue1_p2.png"}, None, {"parent_image": "b/issue2_p1.png"},
             {"parent_image": "issue1_p1.png"}]
    group, page_of, names = rc.duplicate_inputs(metas, "parent")
    assert names == ["issue1_p1.png", "issue1_p2.png", "issue2_p1.png"] and page_of.tolist() == [0, 1, -1, 2, 0]
    assert group.tolist() == [0, 1, -3, 2, 0] and group.dtype == np.int32 and page_of.dtype == np.int32
    group, page_of, _ = rc.duplicate_inputs(metas, "prefix", prefix_length=6)
    assert group.tolist() == [0, 0, -3, 1, 0] and page_of.tolist() == [0, 1, -1, 2, 0]
    assert rc.duplicate_inputs(metas, "none")[0] is None
    with pytest.raises(ValueError):
        rc.duplicate_inputs(metas, "page")


def test_threshold_has_no_default():
    import inspect

    for fn in (rc.duplicate_groups, rc.create_duplicate_report):
        assert inspect.signature(fn).parameters["threshold"].default is inspect.Parameter.empty
