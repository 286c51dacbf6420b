"""K13 (`nms_pages`, csrc/nms.hip, through Engine.nms_boxes) on pages that each decide their result on one named rule, at
the kernel's own limit of 32768 boxes, and with many pages in one call.

Reference: `oracle.regions.nms_keep` (3_combine_grids.py:44-137, float64 in its operation order).  The kept indices and
their order are compared exactly.  All planted coordinates are integers and all scores dyadic or exactly representable, so
every IoU is the exact f64 quotient of two small integers.

Planted pages (geometry_reference.nms_planted_pages; the rule is stated beside each):
  IoU exactly on the threshold -- [0,0,4,4] / [0,0,4,2] (IoU 1/2) kept at 0.5, the second dropped at nextafter(0.5, 0);
    [0,0,2,2] / [1,0,3,2] (IoU 2/6) kept at the f64 value 2/6, dropped one ulp below it;
  greedy chain -- [0,0,10,10], [4,0,14,10], [8,0,18,10] at 0.4 keep [0, 2]: the suppressed middle box suppresses nothing;
  touching and empty boxes -- boxes that share an edge or a corner (IoU 0 through the area branch), a box disjoint on both
    axes (0 through the early return; its two negative extents would multiply to a positive overlap), a zero-area box, an
    inverted box and a repeated zero-area box (union <= 0): all kept at threshold 0.0; at -0.1 (accepted: only NaN is
    refused) IoU 0 exceeds the threshold and the first box drops every other box of its class, disjoint ones included;
  identical boxes at 0.95 (one kept) and at 1.0 (all kept: IoU 1 is not > 1);
  the same box in classes {-2^31, -1, 0, 7, 2^31 - 1}: all kept;
  ties -- all scores equal at n = 255, 256, 257, 1025 (one stride of the 256 lanes and more: kept in index order);
    0.0 against -0.0 (a tie); +inf and -inf (ordered like any score).
Scale: one page of 32768 boxes in 100 clusters, 100 kept, index 32767 kept and 32736..32766 suppressed (the last word of the
bit set); one page of 4096 disjoint boxes, all kept in score order; 32769 boxes refused by name and the next call works.
Many pages: 300 filler pages of 0..300 boxes (every fifth empty) against the oracle in one call; every planted page alone,
first, last and in the middle of those 300.

Mutants (tests/test_geometry_reference_cpu.py asserts each to change the kept list of the pages that name it): `>=` for `>`;
suppression by a higher-scoring box whether kept or not; class ignored; the last of equal scores first; no early return
for disjoint boxes; union without `- inter`; a bit set of 512 words.  "Early return for touching boxes" (`<=` for `<`) is
an equivalent mutant -- the area branch gives the same 0 -- and is asserted there to change nothing.

Measured on the MI355X: whole module 3.4 s (2.1 s of it imports, the first engine and the fillers' oracle).  The
32768-box call alone takes 0.29 s (its test 0.42 s with the oracle's 0.12 s), so the 300-page batches stay as they are; the
two 4096-box calls 0.2 s together; the 30 calls with 300 filler pages 0.03 s together; every planted page below 0.01 s.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from multimodal_embeddings_amd._lib import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def filler():
    pages = G.nms_filler_pages()
    return pages, [G.nms_oracle(p) for p in pages]  # computed once, at the fillers' threshold 0.5


def _run(engine, pages, thr):
    return [k.tolist() for k in engine.nms_boxes(*G.nms_batch(pages), thr)]


@pytest.mark.parametrize("page", G.nms_planted_pages(), ids=lambda p: p["name"].replace(" ", "_"))
def test_planted_page_alone(engine, page):
    want = G.nms_oracle(page)
    if page["expect"] is not None:
        assert want == page["expect"]
    assert _run(engine, [page], page["thr"]) == [want], (page["name"], page["rule"])


def test_negative_threshold_is_accepted(engine):
    page = next(p for p in G.nms_planted_pages() if p["name"] == "touching and empty below 0")
    assert page["thr"] == -0.1 and _run(engine, [page], -0.1) == [[0, 5]]
    assert _run(engine, [page], -np.inf) == [[0, 5]] and _run(engine, [page], np.inf) == [list(range(7))]


def test_32768_boxes_in_one_page(engine):
    page = G.nms_scale_page()
    want = G.nms_oracle(page)
    batch = G.nms_batch([page])
    t0 = time.perf_counter()
    got = engine.nms_boxes(*batch, page["thr"])
    dt = time.perf_counter() - t0
    print(f"32768-box call: {dt:.3f} s, {len(got[0])} kept")
    assert got[0].tolist() == want and want[0] == 32767 and [i for i in want if i >= 32736] == [32767]


def test_4096_boxes_all_kept(engine):
    page = G.nms_all_kept_page()
    want = G.nms_oracle(page)
    assert len(want) == 4096
    assert _run(engine, [page], page["thr"]) == [want]
    one_class_each = dict(page, classes=np.arange(4096, dtype=np.int32), boxes=np.tile(page["boxes"][:1], (4096, 1)))
    assert _run(engine, [one_class_each], 0.5) == [want]  # the same box 4096 times, one class each: the same order


def test_32769_boxes_are_refused_by_name_and_the_next_call_works(engine):
    from multimodal_embeddings_amd._lib import MmeError

    n = G.NMS_MAX_BOXES + 1
    with pytest.raises(MmeError, match="page 1 has 32769 boxes"):
        engine.nms_boxes(np.zeros((n + 2, 4)), np.zeros(n + 2), np.zeros(n + 2, np.int32), [0, 2, n + 2], 0.5)
    chain = next(p for p in G.nms_planted_pages() if p["name"] == "greedy chain")
    assert _run(engine, [chain], chain["thr"]) == [[0, 2]]


def test_300_pages_in_one_call(engine, filler):
    pages, want = filler
    assert _run(engine, pages, 0.5) == want


def test_planted_pages_first_last_and_in_the_middle_of_a_batch(engine, filler):
    pages, want_fill = filler
    planted = G.nms_planted_pages()
    for thr in sorted({p["thr"] for p in planted}):
        group = [p for p in planted if p["thr"] == thr]
        want = [G.nms_oracle(p) for p in group]
        k = len(group)
        for name, batch, at in (("first", group + pages, 0), ("last", pages + group, len(pages)), ("middle", pages[:150] + group + pages[150:], 150)):
            got = _run(engine, batch, thr)
            assert got[at : at + k] == want, (thr, name)
            if thr == 0.5:
                assert got[:at] + got[at + k :] == want_fill, (thr, name)
