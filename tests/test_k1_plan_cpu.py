"""K1's host plan (csrc/k1_plan.h, seen through mme_k1_plan) against tests/k1_plan_reference.py over EVERY size the ABI admits:
1..8000 x 1..8000, one row of 8000 widths per call, for each rule of k1_plan_reference.RULES; the tile geometries of
geometry_reference.OTHER_GEOMETRIES over every pair of a boundary set.  No device is needed: the export is a host function.

One sweep per rule (cached for the module) checks, per size: the resized size and window origin; which passes run; the table
capacities against Resample.c's ksize; the CLIP rule's source-row window; the limits that make an entry point fail (LDS of
either launch, the 160 taps of the vertical pass); class, rows and number of the horizontal pass's bands; bytes and offsets.
The same sweep yields the extreme shapes of the rule, which tests/golden/k1_extreme_shapes.json commits (names and sizes only)
and tests/test_gpu_k1_extremes.py runs on the device; the list is asserted to be exactly what the sweep yields.

Wall time on the development machine: 3 min 14 s to 3 min 51 s for the module, 22-30 s per rule of the full domain (a row of 8000 sizes costs
0.04 ms in the library and about 3 ms of numpy in the reference and the comparisons).  Everything runs on the full domain except the
true-window check (every coordinate of an axis), which runs on the axis pairs the rules reach with at most 224 output
coordinates, and the band lists, which the issue asks for on a thinned set.
"""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import geometry_reference as geo  # noqa: E402
import k1_plan_reference as kref  # noqa: E402
import resize_spec_reference as rsr  # noqa: E402
from multimodal_embeddings_amd._lib import EXPORTS, K1_RECORD, Engine, MmeError  # noqa: E402
from multimodal_embeddings_amd.build import build  # noqa: E402
from oracle import preprocess as opre  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "k1_extreme_shapes.json")
N = 8000
W_ALL = np.arange(1, N + 1, dtype=np.int64)
PIXEL_CAP = 4_000_000  # what the GPU test's Python references can afford per shape
STATES = ("kept", "enlarged", "reduced")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build()


def _first_bad(ok, h, w):
    i = int(np.flatnonzero(~ok)[0])
    return f"at (h, w) = ({int(np.broadcast_to(h, ok.shape)[i])}, {int(np.broadcast_to(w, ok.shape)[i])})"


def _eq(what, got, want, h, w):
    ok = np.asarray(got) == np.asarray(want)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: plan {np.asarray(got)[i]} != reference {np.asarray(want)[i]} {_first_bad(ok, h, w)}")


def _true(what, ok, h, w):
    if not np.all(ok):
        raise AssertionError(f"{what} {_first_bad(np.asarray(ok), h, w)}")


def check(rule, rec, tot, h, w, ref, refusals=False):
    """Every per-size invariant of the issue on one batch.  `ref` = kref.reference(rule, h, w[, mutant])."""
    spec, tiles = rule[0] == "spec", rule[0] == "tiles"
    live = np.ones(len(rec), dtype=bool)
    if tiles and refusals:  # refused exactly when the reference's window exceeds the 160 taps
        _eq("refused (tile window > 160 taps)", rec["refused"], np.where(ref["tile_taps"] > kref.MAX_TAPS, 2, 0), h, w)
        live = rec["refused"] == 0
        _eq("the refused crop's window", rec["kv"][~live], ref["tile_taps"][~live], h[~live], w[~live])
    else:
        _eq("refused", rec["refused"], 0, h, w)
    # the record's fields as contiguous int64 arrays (a field of the record array is a view with a 104-byte stride)
    if live.all():
        hl, wl, R = h, w, ref
        rl = {f: rec[f].astype(np.int64) for f in K1_RECORD.names}
    else:
        hl, wl = h[live], w[live]
        rl = {f: rec[f][live].astype(np.int64) for f in K1_RECORD.names}
        R = {k: v[live] for k, v in ref.items()}
    # sizes
    for f in ("new_h", "new_w", "top", "left", "th", "tw"):
        _eq(f, rl[f], R[f], hl, wl)
    # passes: a pass runs exactly when that side changes
    _eq("h_pass", rl["h_pass"], rl["new_w"] != wl, hl, wl)
    _eq("v_pass", rl["v_pass"], rl["new_h"] != hl, hl, wl)
    # capacity
    hp, vp = rl["h_pass"] == 1, rl["v_pass"] == 1
    _true("gh * 4 < ksize", ~hp | (rl["gh"] * 4 >= R["ksize_h"]), hl, wl)
    _true("kv < ksize", ~vp | (rl["kv"] >= R["ksize_v"]), hl, wl)
    _true("kv % 4", rl["kv"] % 4 == 0, hl, wl)
    _eq("gh (ksize rounded up to groups of four)", rl["gh"], R["gh"], hl, wl)
    _eq("kv (ksize rounded up to four)", rl["kv"], R["kv"], hl, wl)
    # the CLIP rule's source-row window
    _eq("r0", rl["r0"], R["r0"], hl, wl)
    _eq("nr", rl["nr"], R["nr"], hl, wl)
    if spec:
        sup = kref.SUPPORT[rule[1].resample]
        _true("r0 < 0 or r0 + nr > h", (rl["r0"] >= 0) & (rl["r0"] + rl["nr"] <= hl), hl, wl)
        # windows move monotonically with the output coordinate (center grows, support is fixed, int() and the clamps are
        # monotone): the first row's xmin and the last row's xmax bound all 224 (every row is checked on the reached pairs
        # with at most 224 rows, test_true_windows_fit_the_capacity, and on a thinned set, test_clip_window_holds_every_row)
        lo, _ = kref.window(hl, rl["new_h"], rl["top"], sup)
        _, hi = kref.window(hl, rl["new_h"], rl["top"] + kref.SIZE - 1, sup)
        _true("a vertical window outside [r0, r0 + nr)", ~vp | ((rl["r0"] <= lo) & (hi <= rl["r0"] + rl["nr"])), hl, wl)
        _true("height kept: rows top..top + 223", vp | ((rl["r0"] == rl["top"]) & (rl["nr"] == kref.SIZE)), hl, wl)
    # limits: no admitted crop makes an entry point fail
    _true("horizontal LDS request > 160 KiB", rl["h_lds"] <= kref.LDS_LIMIT, hl, wl)
    _eq("h_lds", rl["h_lds"], R["h_lds"], hl, wl)
    if not tiles:
        _true("kv > MAX_TAPS", rl["kv"] <= kref.MAX_TAPS, hl, wl)
        _eq("v_lds", rl["v_lds"], 16 * np.maximum(rl["kv"], 4) * 4 + 16 * 1024 + 1024, hl, wl)
        _true("vertical LDS beyond what a workgroup may hold", rl["v_lds"] + kref.V_STATIC_LDS <= kref.LDS_LIMIT, hl, wl)
    # bands
    _eq("h_class", rl["h_class"], R["cls"], hl, wl)
    _eq("band_rows", rl["band_rows"], R["band_rows"], hl, wl)
    _eq("n_bands", rl["n_bands"], R["n_bands"], hl, wl)
    c0 = rl["h_class"] == 0
    _true("class 0 rows", ~c0 | ((rl["band_rows"] % 8 == 0) & (rl["band_rows"] <= 64) & (rl["band_rows"] >= 8)), hl, wl)
    _true("class 1, 2 rows", ~(rl["h_class"] >= 1) | (rl["band_rows"] == 4), hl, wl)
    # bytes and offsets: 16-byte aligned, one after the other (so disjoint), totals = the sums, every count in its type
    want_tmp = rl["nr"] * 672 if spec else np.where(hp, hl * kref.pad(rl["new_w"] * 3, 16), 0)
    _eq("tmp_bytes", rl["tmp_bytes"], want_tmp, hl, wl)
    for off, size in (("tab_off", "tab_bytes"), ("tmp_off", "tmp_bytes")):
        _true(f"{size} % 16", rl[size] % 16 == 0, hl, wl)
        sizes = np.where(live, rec[size], 0)
        start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        used = live & (rec[size] > 0)
        _eq(off, rec[off][used], start[used], h[used], w[used])
    assert tot[0] == rl["tab_bytes"].sum() and tot[1] == rl["tmp_bytes"].sum() and tot[2] == rl["n_bands"].sum() < 2 ** 31
    assert tot[3] == (rl["kv"].max() if len(hl) else 0)
    return R, rl


class Extremes:
    """kind -> (value, -pixels, -h, -w): the largest value, then the fewest pixels, then the smaller h, then the smaller w"""

    def __init__(self):
        self.best = {}

    def take(self, kind, metric, h, w, mask=None):
        """one ROW of the domain: h is one height and w ascends, so the first width attaining the value has the fewest pixels"""
        if mask is None:
            v = metric.max()
            j = int((metric == v).argmax())
        else:
            j = int(mask.argmax())
            if not mask[j]:
                return
            v = 1
        cand = (int(v), -h * int(w[j]), -h, -int(w[j]))
        if kind not in self.best or cand > self.best[kind]:
            self.best[kind] = cand

    def shapes(self):
        return {k: (-v[2], -v[3]) for k, v in self.best.items()}


def _state(n_in, n_out):
    return np.where(n_out == n_in, 0, np.where(n_out > n_in, 1, 2))


def gather(ext, stats, reached, rule, rec, R, h, w):
    """h: the row's height (an int); w: its widths, ascending; rec: the record's fields as `check` returns them"""
    spec = rule[0] == "spec"
    rh, rw = rec["new_h"], rec["new_w"]
    ext.take("largest gh", rec["gh"], h, w)
    ext.take("largest kv", rec["kv"], h, w)
    ext.take("largest horizontal LDS request", rec["h_lds"], h, w)
    ext.take("largest scratch image", rec["tmp_bytes"], h, w)
    for k in (8, 7, 4, 3):
        ext.take(f"fit {k}", None, h, w, R["fit"] == k)
    ext.take("smallest new_h", -rh, h, w)
    ext.take("largest new_h", rh, h, w)
    ext.take("smallest new_w", -rw, h, w)
    ext.take("largest new_w", rw, h, w)
    state = _state(h, rh) * 3 + _state(w, rw)
    for a in range(3):
        for b in range(3):  # "height reduced / enlarged, width kept" is form (c) of resize_v_patchify with a vertical pass
            ext.take(f"height {STATES[a]}, width {STATES[b]}", None, h, w, state == a * 3 + b)
    if spec:
        ext.take("largest nr", rec["nr"], h, w)
        ext.take("nr == 1", None, h, w, rec["nr"] == 1)
    for name, ch, cw in (("corner 1 x 1", 1, 1), ("corner 1 x 8000", 1, N), ("corner 8000 x 1", N, 1), ("corner 8000 x 8000", N, N)):
        if ch * cw <= PIXEL_CAP and h == ch:
            ext.take(name, None, h, w, w == cw)
    for k, v in (("gh", rec["gh"]), ("kv", rec["kv"]), ("tab_bytes", rec["tab_bytes"]), ("tmp_bytes", rec["tmp_bytes"]), ("h_lds", rec["h_lds"]),
                 ("ksize", np.maximum(R["ksize_h"], R["ksize_v"])), ("class 2 band", np.where(rec["h_class"] == 2, rec["h_lds"] - 64 - 1024, 0))):
        stats[k] = max(stats.get(k, 0), int(v.max()))
    # axis pairs reached with at most 224 output coordinates (a spec's window then starts at coordinate 0)
    sup = kref.SUPPORT[rule[1].resample] if spec else 1.0
    for n_in, n_out, run in ((w, rw, rec["h_pass"] == 1), (h, rh, rec["v_pass"] == 1)):
        m = run & (n_out <= kref.SIZE)
        reached.setdefault(sup, np.zeros((N + 1, kref.SIZE + 1), dtype=bool))[np.broadcast_to(n_in, m.shape)[m], n_out[m]] = True


_SWEEPS = {}


def sweep(name):
    """the whole domain of one rule, checked; -> (extreme shapes, attained maxima, reached axis pairs)"""
    if name not in _SWEEPS:
        rule = kref.RULES[name]
        arg, kw = kref.engine_rule(rule)
        ext, stats, reached = Extremes(), {}, {}
        hw = np.empty((N, 2), dtype=np.int32)
        hw[:, 1] = W_ALL
        for hh in range(1, N + 1):
            hw[:, 0] = hh
            h = np.full(N, hh, dtype=np.int64)
            rec, tot = Engine.k1_plan(arg, hw, **kw)
            R, fields = check(rule, rec, tot, h, W_ALL, kref.reference(rule, h, W_ALL))
            gather(ext, stats, reached, rule, fields, R, hh, W_ALL)
        _SWEEPS[name] = (ext.shapes(), stats, reached)
    return _SWEEPS[name]


def test_the_export_is_declared_and_the_record_is_the_headers():
    header = open(os.path.join(ROOT, "include", "mme.h")).read()
    assert "#define MME_ABI_VERSION 2\n" in header, "an export is added, none changes"
    assert "int mme_k1_plan(const mme_k1_rule* rule, const int32_t* hw_host, int n, mme_k1_record* out, int64_t totals[4], int32_t* bands_host," in header
    assert "mme_k1_plan" in EXPORTS and len(EXPORTS["mme_k1_plan"][1]) == 7
    body = header[header.index("typedef struct mme_k1_record {"):header.index("} mme_k1_record;")]
    import re

    fields = [f.strip() for decl in re.findall(r"int(?:32|64)_t ([a-z0-9_, ]+);", body) for f in decl.split(",")]
    assert fields == list(K1_RECORD.names) and K1_RECORD.itemsize == 18 * 4 + 4 * 8
    # the alignment rule is stated once, and the sentence at mme_crop_boxes no longer asks for aligned crops
    assert header.count("THE ALIGNMENT RULE") == 1 and "16-byte aligned crops" not in header
    with pytest.raises(MmeError, match=r"mme_k1_plan: spec \{mode 0, height 223"):
        Engine.k1_plan(kref.ResizeSpec("shortest_edge", 223, 0, 3), [[1, 1]])
    with pytest.raises(MmeError, match=r"mme_k1_plan: need tile in 8\.\.1024"):
        Engine.k1_plan("tiles", [[1, 1]], tile=12)
    rec, _ = Engine.k1_plan("fit_pad", [[0, 5], [8001, 1], [5, 5]])
    assert rec["refused"].tolist() == [1, 1, 0] and rec["tab_off"][2] == 0


def test_the_vectorised_reference_is_the_scalar_definitions():
    """k1_plan_reference's array forms against the functions they restate, on a boundary set of sizes"""
    B = kref.boundary_set(224)[::3].tolist() + [223, 224, 225, 447, 448, 449, 7999, 8000]
    hh, ww = (a.ravel() for a in np.meshgrid(np.array(B), np.array(B[::5] + [224, 8000]), indexing="ij"))
    nh, nw = kref.fit_sizes(hh, ww)
    th, tw, t_nh, t_nw = kref.tile_sizes(hh, ww, 560, 4)
    specs = {k: kref.spec_sizes(r[1], hh, ww) for k, r in kref.RULES.items() if r[0] == "spec"}
    R = kref.reference(kref.RULES["fit_pad"], hh, ww)
    for i, (h, w) in enumerate(zip(hh.tolist(), ww.tolist())):
        assert (nh[i], nw[i]) == opre.fit_to_canvas(h, w), (h, w)
        assert (th[i], tw[i], t_nh[i], t_nw[i]) == geo.tile_geometry(h, w, 560, 4), (h, w)
        for k, s in specs.items():
            assert tuple(int(a[i]) for a in s) == rsr.spec_geometry(kref.RULES[k][1], h, w), (k, h, w)
        assert kref.CLASS_NAMES[int(R["cls"][i])] == geo.h_pass_class(w, int(nw[i])), (h, w)
        for n_in, n_out, k in ((w, int(nw[i]), R["ksize_h"][i]), (h, int(nh[i]), R["ksize_v"][i])):
            assert k == (geo.window_taps(n_in, n_out) if n_in != n_out else 0), (h, w)


@pytest.mark.parametrize("name", list(kref.RULES))
def test_the_plan_over_the_whole_domain(name):
    shapes, stats, _ = sweep(name)
    rule = kref.RULES[name]
    if rule[0] == "tiles":
        assert stats["kv"] <= 20, "at (560, 4) the scale is at least 1120 / 8000: never near the 160 taps"


def test_the_bounds_the_comments_state_are_the_attained_maxima():
    """csrc/k1_plan.h, resample.h: every figure in a comment about the spec path is attained over the swept specs, and the
    fit-and-pad figures are the attained ones"""
    spec = [sweep(k)[1] for k, r in kref.RULES.items() if r[0] == "spec"]
    top = {k: max(s[k] for s in spec) for k in spec[0]}
    assert (top["ksize"], top["gh"], top["kv"], top["tab_bytes"], top["tmp_bytes"], top["class 2 band"]) == (145, 37, 148, 268800, 5376000, 4 * 24000)
    fit = sweep("fit_pad")[1]
    assert (fit["ksize"], fit["gh"], fit["kv"], fit["tmp_bytes"], fit["class 2 band"]) == (143, 36, 144, 5376000, 4 * 24000)
    text = open(os.path.join(ROOT, "multimodal_embeddings_amd", "csrc", "k1_plan.h")).read()
    assert f"tables take <= {fit['tab_bytes']:,}".replace(",", " ") in text, fit["tab_bytes"]
    assert max(s["h_lds"] for s in spec + [fit, sweep("tiles560")[1]]) == 4 * 24000 + 64 + 1024 <= kref.LDS_LIMIT


def test_true_windows_fit_the_capacity():
    """For every axis pair some rule reaches with at most 224 output coordinates: the longest window Resample.c's xmin / xmax
    give over ALL its coordinates is within ksize, hence within the capacity the sweep held equal to ksize rounded up."""
    reached = {}
    for name in kref.RULES:
        for sup, m in sweep(name)[2].items():
            reached[sup] = reached.get(sup, False) | m
    pairs = 0
    for sup, m in reached.items():
        for n_out in range(1, kref.SIZE + 1):
            n_in = np.flatnonzero(m[:, n_out])
            if not len(n_in):
                continue
            pairs += len(n_in)
            lo, hi = kref.window(n_in[:, None], n_out, np.arange(n_out)[None, :], sup)
            longest = (hi - lo).max(axis=1)
            _true(f"a window longer than ksize (support {sup}, out {n_out})", longest <= kref.ksize(n_in, n_out, sup), n_in, n_out)
            assert (lo[:, 1:] >= lo[:, :-1]).all() and (hi[:, 1:] >= hi[:, :-1]).all(), "windows move monotonically"
    assert pairs > 100_000


def test_clip_window_holds_every_row():
    """all 224 rows' windows, not only the first and the last, on a boundary set of sizes under every spec"""
    B = kref.boundary_set(224)
    hh, ww = (a.ravel() for a in np.meshgrid(B, B[::7], indexing="ij"))
    for name, rule in kref.RULES.items():
        if rule[0] != "spec":
            continue
        rec, _ = Engine.k1_plan(rule[1], np.stack([hh, ww], 1))
        vp = rec["v_pass"] == 1
        h, r = hh[vp], rec[vp]
        lo, hi = kref.window(h[:, None], r["new_h"][:, None], r["top"][:, None] + np.arange(kref.SIZE)[None, :], kref.SUPPORT[rule[1].resample])
        assert (lo.min(axis=1) == r["r0"]).all() and (np.maximum(hi.max(axis=1), r["r0"] + 1) == r["r0"] + r["nr"]).all(), name
        assert ((hi - lo).max(axis=1) <= r["kv"]).all(), name


@pytest.mark.parametrize("tile,max_tiles", geo.OTHER_GEOMETRIES)
def test_other_tile_geometries_on_their_boundary_sets(tile, max_tiles):
    rule = ("tiles", tile, max_tiles)
    B = kref.boundary_set(tile)
    refused = 0
    for hh in B.tolist():
        h = np.full(len(B), hh, dtype=np.int64)
        rec, tot = Engine.k1_plan("tiles", np.stack([h, B], 1), tile=tile, max_tiles=max_tiles)
        check(rule, rec, tot, h, B, kref.reference(rule, h, B), refusals=True)
        refused += int((rec["refused"] != 0).sum())
    # 8000 x 8000 fills the squarest canvas, isqrt(max_tiles) tiles high: refused where that is a reduction by more than 79
    assert (refused > 0) == (8000 > 79 * tile * math.isqrt(max_tiles))


def test_the_band_lists_cover_every_source_row_once_and_in_order():
    hs = np.array([1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 71, 127, 128, 129, 224, 225, 300, 1000, 7999, 8000])
    ws = kref.boundary_set(224)[::4]
    hh, ww = (a.ravel() for a in np.meshgrid(hs, ws, indexing="ij"))
    assert 2000 < len(hh) < 10000
    for name, rule in kref.RULES.items():
        arg, kw = kref.engine_rule(rule)
        for part in np.array_split(np.arange(len(hh)), 40):  # batches of ~ 60 mixed sizes
            h, w = hh[part], ww[part]
            rec, tot, bands = Engine.k1_plan(arg, np.stack([h, w], 1), bands=True, **kw)
            R = kref.reference(rule, h, w)
            assert len(bands) == tot[2] == R["n_bands"].sum()
            assert (np.diff(bands[:, 3]) >= 0).all(), "class 0 | class 1 | class 2"
            order = np.lexsort((np.arange(len(bands)), bands[:, 0]))  # by crop, launch order kept
            b = bands[order]
            for i in range(len(h)):
                mine = b[b[:, 0] == i]
                assert len(mine) == rec["n_bands"][i] and (mine[:, 3] == rec["h_class"][i]).all(), (name, h[i], w[i])
                if not len(mine):
                    assert R["nrows"][i] == 0
                    continue
                first = rec["r0"][i] if rule[0] == "spec" else 0
                assert mine[0, 1] == first and (mine[1:, 1] == mine[:-1, 1] + mine[:-1, 2]).all(), (name, h[i], w[i])
                assert mine[-1, 1] + mine[-1, 2] == first + R["nrows"][i], (name, h[i], w[i])
                assert (mine[:-1, 2] == rec["band_rows"][i]).all() and 1 <= mine[-1, 2] <= rec["band_rows"][i], (name, h[i], w[i])


def test_random_batches_keep_offsets_aligned_and_disjoint():
    rng = np.random.default_rng(61)
    for name, rule in kref.RULES.items():
        arg, kw = kref.engine_rule(rule)
        for _ in range(200):
            n = int(rng.integers(1, 65))
            hw = np.where(rng.random((n, 2)) < 0.3, rng.integers(1, 300, (n, 2)), rng.integers(1, N + 1, (n, 2)))
            rec, tot = Engine.k1_plan(arg, hw, **kw)
            check(rule, rec, tot, hw[:, 0], hw[:, 1], kref.reference(rule, hw[:, 0], hw[:, 1]))
            for off, size in (("tab_off", "tab_bytes"), ("tmp_off", "tmp_bytes")):
                used = rec[rec[size] > 0]  # a crop without a scratch image has offset 0 and no bytes
                assert (used[off] % 16 == 0).all() and (used[off][1:] >= used[off][:-1] + used[size][:-1]).all()
                assert (used[off][-1] + used[size][-1] if len(used) else 0) == tot[0 if off == "tab_off" else 1] < 2 ** 40


@pytest.mark.parametrize("mutant,name", [("ksize_without_plus_one", "fit_pad"), ("ksize_without_plus_one", "clip"), ("class_budget_64k", "fit_pad"),
                                         ("class_budget_64k", "clip"), ("r0_from_top_plus_one", "clip")])
def test_the_invariants_have_teeth(mutant, name):
    """each deliberately wrong restatement is caught on at least one size (and the right one on none of the same sizes)"""
    rule = kref.RULES[name]
    arg, kw = kref.engine_rule(rule)
    caught = 0
    for hh in (1, 100, 224, 225, 300, 1000, 3000, 8000):
        h = np.full(N, hh, dtype=np.int64)
        rec, tot = Engine.k1_plan(arg, np.stack([h, W_ALL], 1), **kw)
        check(rule, rec, tot, h, W_ALL, kref.reference(rule, h, W_ALL))
        try:
            check(rule, rec, tot, h, W_ALL, kref.reference(rule, h, W_ALL, mutant))
        except AssertionError:
            caught += 1
    assert caught >= 1


def derive_extremes():
    """{rule: [{"kind", "h", "w"[, "over_4M"]}]} from the sweeps: what tests/golden/k1_extreme_shapes.json holds"""
    out = {}
    for name in kref.RULES:
        rows = []
        for kind, (h, w) in sorted(sweep(name)[0].items()):
            row = {"kind": kind, "h": h, "w": w}
            if h * w > PIXEL_CAP:
                row["over_4M"] = True  # attained by no smaller shape: kept, and the GPU test pays for it
            rows.append(row)
        out[name] = rows
    return out


def test_the_committed_extreme_shapes_are_what_the_sweep_yields():
    want = derive_extremes()
    got = json.load(open(GOLDEN))
    assert got["rules"] == want, "regenerate tests/golden/k1_extreme_shapes.json from derive_extremes()"
    for name, rows in want.items():
        kinds = {r["kind"] for r in rows}
        need = {"largest gh", "largest kv", "largest horizontal LDS request", "largest scratch image", "smallest new_h", "largest new_h", "smallest new_w",
                "largest new_w", "corner 1 x 1", "corner 1 x 8000", "corner 8000 x 1"}
        assert need <= kinds, (name, need - kinds)
    fit = {r["kind"] for r in want["fit_pad"]}
    assert {"fit 8", "fit 7", "fit 4", "fit 3", "height reduced, width kept", "height enlarged, width kept"} <= fit
    assert {"largest nr", "nr == 1"} <= {r["kind"] for r in want["clip"]}
