// K1's host planning: the size rules of the three resize rules (fit-and-pad, resize spec, Mllama tile canvas), the per-crop
// plan (tables, scratch image, the CLIP rule's source-row window) and the bands of the horizontal pass.  Pure integer / f64
// host arithmetic: no HIP runtime call and no context, so the whole admitted domain (1..8000 x 1..8000 per rule) is swept
// on a machine without a GPU -- through mme_k1_plan (capi.hip) by tests/test_k1_plan_cpu.py and, under a sanitizer, by
// tools/k1_plan_sweep.cpp.  The entry points of capi.hip plan with these functions and no others.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mme.h"
#include "resample.h"

// Mllama single-tile fit (transformers image_processing_pil_mllama.py:246-295, canvas == tile)
inline void fit_to_canvas(int h, int w, int* nh, int* nw) {
    const double scale_h = (double)VIT_IMG / h, scale_w = (double)VIT_IMG / w;
    if (scale_w < scale_h) {
        *nw = VIT_IMG;
        int v = (int)std::floor(h * scale_w);
        if (v == 0) v = 1;
        *nh = v < VIT_IMG ? v : VIT_IMG;
    } else {
        *nh = VIT_IMG;
        int v = (int)std::floor(w * scale_h);
        if (v == 0) v = 1;
        *nw = v < VIT_IMG ? v : VIT_IMG;
    }
}

// K1 plan shared by the preprocessing entry points: scratch image + resampling tables of every crop and the bands of
// the horizontal pass.  A band is a whole number of row groups (the rows one work item filters).  Three classes, one
// launch each:
//   0  table + eight rows fit kHLds bytes of LDS: eight-row items, table in LDS beside the band (five workgroups per CU at 32 KiB)
//   1  table + four rows fit: four-row items, table in LDS
//   2  wider crops: one four-row group per band, the table read through L1, LDS sized for the widest of them
struct K1Plan {
    size_t tmp_bytes = 0, tab_bytes = 0;
    std::vector<HWork> work[3];
    int lds[3] = {16, 16, 16};  // largest (table +) band per class
    int count[3] = {0, 0, 0};
    int kv_max = 0;  // largest K1Layout::kv of the batch (LDS of the vertical pass)
    // false: plan_bands counts the bands (nbands) and sizes the LDS but lists none (mme_k1_plan over millions of sizes); the
    // entry points leave it true
    bool list_bands = true;
    size_t nbands = 0;
};
// LDS budget of classes 0 and 1
constexpr int kHLds = 32 * 1024;

// The band shape of a crop's horizontal pass, in O(1): nrows source rows of row_bytes each, whose table takes tab_lds bytes
// of LDS when it rides beside the band.  cls: the class; rows: source rows per band (the last band may hold fewer);
// nbands: how many bands; lds: the (table +) band bytes of this crop, what K1Plan::lds takes the class maximum of.
struct BandShape {
    int cls, rows, nbands, lds;
};
inline BandShape band_shape(int row_bytes, int tab_lds, int nrows) {
    const int fit = tab_lds < kHLds ? (kHLds - tab_lds) / row_bytes : 0;  // rows that fit beside the table
    const int cls = fit >= K1_H_RPT ? 0 : (fit >= K1_H_RPT_WIDE ? 1 : 2);
    int rows = cls == 0 ? (fit & ~(K1_H_RPT - 1)) : K1_H_RPT_WIDE;
    if (rows > 64) rows = 64;
    const int bb = (rows < nrows ? rows : nrows) * row_bytes + (cls < 2 ? tab_lds : 0);
    return BandShape{cls, rows, (nrows + rows - 1) / rows, bb};
}
// The bands of crop i's horizontal pass: source rows [first_row, first_row + nrows).  Appends them to their class: the one
// producer of bands.
inline void plan_bands(K1Plan& p, int i, int row_bytes, int tab_lds, int first_row, int nrows) {
    const BandShape b = band_shape(row_bytes, tab_lds, nrows);
    p.nbands += (size_t)b.nbands;
    if (p.list_bands)
        for (int r = 0; r < nrows; r += b.rows) p.work[b.cls].push_back(HWork{i, first_row + r, (nrows - r) < b.rows ? (nrows - r) : b.rows});
    if (b.lds > p.lds[b.cls]) p.lds[b.cls] = b.lds;
}

// Fit-and-pad and tiles: d.h, d.w, d.new_h, d.new_w are set.  Measured over the whole domain (tests/test_k1_plan_cpu.py): under
// fit-and-pad ksize <= 143, gh <= 36 (7841 x 70 becomes one column) and kv <= 144 (70 x 7841 becomes one row), a crop's
// tables take <= 139 776 bytes, its scratch image <= 8000 * 672 = 5 376 000 bytes, and the widest class-2 band is 4 * 24000 bytes.
inline void plan_crop(K1Plan& p, int i, CropDesc& d) {
    d.tmp_off = 0;
    d.tab_off = (int64_t)p.tab_bytes;
    const K1Layout lay = k1_layout(d.h, d.w, d.new_h, d.new_w);
    p.tab_bytes += (size_t)lay.bytes;
    if (lay.kv > p.kv_max) p.kv_max = lay.kv;
    if (d.new_w == d.w) return;
    d.tmp_off = (int64_t)p.tmp_bytes;
    p.tmp_bytes += (size_t)d.h * k1_tmp_pitch(d.new_w);
    plan_bands(p, i, d.w * 3, k1_h_table_lds(d.w, d.new_w), 0, d.h);
}

// ---- K1 under MME_RESIZE_CLIP and MME_RESIZE_SPEC (preprocess_clip.hip) ---------------------------------------------------
// One path serves both: rule 1 is the spec below, what CLIPImageProcessorPil does.
constexpr mme_resize_spec kClipSpec = {MME_RESIZE_MODE_SHORTEST_EDGE, VIT_IMG, 0, 3};
// a 224 x 224 crop is resized to 224 x 224, i.e. not filtered on either axis, and its centre window is the crop
inline bool spec_keeps_canvas(const mme_resize_spec& sp) {
    return sp.mode == MME_RESIZE_MODE_EXACT ? (sp.height == VIT_IMG && sp.width == VIT_IMG) : sp.height == VIT_IMG;
}
// The size of the whole resized image.  EXACT: the spec's.  SHORTEST_EDGE S: transformers image_transforms.py
// get_resize_output_image_size, size = {"shortest_edge": S}, default_to_square = False: the short edge gets S, the long
// edge int(S * long / short) -- the Python float expression in that order, in f64
inline void spec_resized_size(const mme_resize_spec& sp, int h, int w, int* nh, int* nw) {
    if (sp.mode == MME_RESIZE_MODE_EXACT) {
        *nh = sp.height;
        *nw = sp.width;
        return;
    }
    const int sh = h <= w ? h : w, lg = h <= w ? w : h;
    const int nl = (int)((double)(sp.height * (int64_t)lg) / (double)sh);
    *nh = h <= w ? sp.height : nl;
    *nw = h <= w ? nl : sp.height;
}
// Resample.c's ksize (resample.h), the upper bound of a window's taps; 1 for an axis that is not filtered
template <class Filter>
int axis_ksize(int in_size, int out_size) {
    return in_size == out_size ? 1 : resample_ksize<Filter>(in_size, out_size);
}

// Sizes against the 8000 x 8000 limit, resized edges >= 224: ksize <= 2 * ceil(2 * 8000 / 224) + 1 = 145 (BICUBIC; 73 for
// BILINEAR), attained from 7841 source pixels on, so gh <= 37 and kv <= 148 (the vertical pass holds 160); a crop's tables take
// <= 3584 + 37 * 3584 + 224 * 148 * 4 = 268 800 bytes and its scratch image <= 8000 * 672 = 5 376 000 bytes (nr <= h), both
// summed in size_t.  The widest class-2 band is 4 * 24000 bytes of LDS.  All attained (tests/test_k1_plan_cpu.py sweeps the
// whole domain).  Filter = the spec's (Triangle for resample 2, Bicubic for 3).
template <class Filter>
void plan_spec_crop(K1Plan& p, int i, ClipCropDesc& d, const mme_resize_spec& sp) {
    spec_resized_size(sp, d.h, d.w, &d.new_h, &d.new_w);
    d.top = (d.new_h - VIT_IMG) / 2;
    d.left = (d.new_w - VIT_IMG) / 2;
    if (d.new_h != d.h) {
        // the union of the 224 vertical windows: the expressions clip_tables evaluates on the device (resample.h); the
        // whole source height when the window is the whole resized image (an exact 224 target)
        const Taps first = resample_window<Filter>(d.h, d.new_h, d.top), last = resample_window<Filter>(d.h, d.new_h, d.top + VIT_IMG - 1);
        const int a = first.xmin, z = last.xmin + last.n;
        d.r0 = a;
        d.nr = (z > a ? z : a + 1) - a;
    } else {
        d.r0 = d.top;
        d.nr = VIT_IMG;
    }
    d.gh = (axis_ksize<Filter>(d.w, d.new_w) + 3) >> 2;
    d.kv = (axis_ksize<Filter>(d.h, d.new_h) + 3) & ~3;
    if (d.kv > p.kv_max) p.kv_max = d.kv;
    d.tab_off = (int64_t)p.tab_bytes;
    p.tab_bytes += (size_t)clip_layout(d.gh, d.kv).bytes;
    d.tmp_off = (int64_t)p.tmp_bytes;
    p.tmp_bytes += (size_t)d.nr * (VIT_IMG * 3);
    plan_bands(p, i, d.w * 3, clip_h_table_lds(d.gh), d.r0, d.nr);
}
inline void plan_spec_crop(K1Plan& p, int i, ClipCropDesc& d, const mme_resize_spec& sp) {
    if (sp.resample == 2)
        plan_spec_crop<Triangle>(p, i, d, sp);
    else
        plan_spec_crop<Bicubic>(p, i, d, sp);
}

// ---- Mllama tile canvas (transformers image_processing_pil_mllama.py:216-355), f64 like numpy ----
inline void optimal_tile_grid(int h, int w, int max_tiles, int tile, int* th, int* tw) {
    // supported grids (a, b), a outer / b inner (:216-243), treated as (tiles_h, tiles_w) (:329-332)
    int ga[64], gb[64], ng = 0;
    double sc[64];
    for (int a = 1; a <= max_tiles; ++a)
        for (int b = 1; b <= max_tiles; ++b)
            if (a * b <= max_tiles && ng < 64) {
                const double sh = (double)(a * tile) / (double)h, sw = (double)(b * tile) / (double)w;
                ga[ng] = a;
                gb[ng] = b;
                sc[ng++] = sw > sh ? sh : sw;  // np.where(scale_w > scale_h, scale_h, scale_w)
            }
    bool any_up = false;
    double sel = 0.0;
    for (int i = 0; i < ng; ++i)
        if (sc[i] >= 1.0 && (!any_up || sc[i] < sel)) {  // smallest upscaling factor (:337-339)
            sel = sc[i];
            any_up = true;
        }
    if (!any_up) {
        bool first = true;
        for (int i = 0; i < ng; ++i)
            if (first || sc[i] > sel) {  // largest downscaling factor (:340-343)
                sel = sc[i];
                first = false;
            }
    }
    long best_area = -1;
    for (int i = 0; i < ng; ++i)
        if (sc[i] == sel) {  // ties: smallest canvas area, first in list order (:346-353)
            const long area = (long)(ga[i] * tile) * (long)(gb[i] * tile);
            if (best_area < 0 || area < best_area) {
                best_area = area;
                *th = ga[i];
                *tw = gb[i];
            }
        }
}

inline void fit_to_tile_canvas(int h, int w, int canvas_h, int canvas_w, int tile, int* nh, int* nw) {
    const int target_w = w < tile ? tile : (w > canvas_w ? canvas_w : w);
    const int target_h = h < tile ? tile : (h > canvas_h ? canvas_h : h);
    const double scale_h = (double)target_h / (double)h, scale_w = (double)target_w / (double)w;
    if (scale_w < scale_h) {
        *nw = target_w;
        int v = (int)std::floor((double)h * scale_w);
        if (v == 0) v = 1;
        *nh = v < target_h ? v : target_h;
    } else {
        *nh = target_h;
        int v = (int)std::floor((double)w * scale_h);
        if (v == 0) v = 1;
        *nw = v < target_w ? v : target_w;
    }
}

// The tile grid and the resized size of a crop (d.h, d.w set) under (tile, max_tiles).  Returns 0, or the taps of the vertical
// window where they exceed MAX_TAPS: resize_v_tiles holds a row's vertical taps in MAX_TAPS words of LDS; a longer window
// would be cut short there (wrong pixels, no error), so such a batch is refused whole, before anything is launched.  The
// horizontal pass sizes its table from the crop and has no such limit.
inline int tile_crop_size(CropDesc& d, int tile, int max_tiles, int* th, int* tw) {
    *th = 1;
    *tw = 1;
    optimal_tile_grid(d.h, d.w, max_tiles, tile, th, tw);
    fit_to_tile_canvas(d.h, d.w, *th * tile, *tw * tile, tile, &d.new_h, &d.new_w);
    if (d.new_h != d.h) {
        const int window = resample_ksize<Triangle>(d.h, d.new_h);
        if (window > MAX_TAPS) return window;
    }
    return 0;
}

// ---- the host's view of a batch's plan (mme_k1_plan) ---------------------------------------------------------------------
// what mme_set_resize_spec and mme_preprocess_tiles admit
inline bool spec_admitted(const mme_resize_spec& sp) {
    const bool exact = sp.mode == MME_RESIZE_MODE_EXACT;
    if (sp.mode != MME_RESIZE_MODE_SHORTEST_EDGE && !exact) return false;
    if (sp.height < VIT_IMG || sp.height > 512) return false;
    if (exact ? (sp.width < VIT_IMG || sp.width > 512) : sp.width != 0) return false;
    return sp.resample == 2 || sp.resample == 3;
}
inline bool tiles_admitted(int tile, int max_tiles) { return !(tile < 8 || tile > 1024 || (tile % 8) != 0 || max_tiles < 1 || max_tiles > 16); }
inline bool crop_size_admitted(int h, int w) { return !(h <= 0 || w <= 0 || h > 8000 || w > 8000); }

// One record per crop of a batch, from the plan the entry point of the rule builds (plan_crop / plan_spec_crop and, through
// them, plan_bands: `p` holds the bands afterwards).  The band fields restate nothing: band_shape is what plan_bands appended
// from.  A refused crop takes no part in the plan.
inline void k1_plan_records(const mme_k1_rule& rule, const int32_t* hw, int n, mme_k1_record* out, K1Plan& p) {
    for (int i = 0; i < n; ++i) {
        mme_k1_record r{};
        const int h = hw[2 * i], w = hw[2 * i + 1];
        r.th = r.tw = 1;
        r.h_class = -1;
        if (!crop_size_admitted(h, w)) {
            r.refused = MME_K1_REFUSED_SIZE;
            out[i] = r;
            continue;
        }
        const size_t tab0 = p.tab_bytes, tmp0 = p.tmp_bytes;
        int row_bytes = w * 3, tab_lds = 0, nrows = 0;
        if (rule.kind == MME_K1_RULE_SPEC) {
            ClipCropDesc d{};
            d.h = h;
            d.w = w;
            plan_spec_crop(p, i, d, rule.spec);
            r.new_h = d.new_h, r.new_w = d.new_w, r.top = d.top, r.left = d.left, r.r0 = d.r0, r.nr = d.nr;
            r.gh = d.gh, r.kv = d.kv;
            r.tab_off = d.tab_off, r.tmp_off = d.tmp_off;
            tab_lds = clip_h_table_lds(d.gh);
            nrows = d.nr;
        } else {
            CropDesc d{};
            d.h = h;
            d.w = w;
            if (rule.kind == MME_K1_RULE_TILES) {
                int th, tw;
                const int window = tile_crop_size(d, rule.tile, rule.max_tiles, &th, &tw);
                r.th = th, r.tw = tw;
                if (window) {
                    r.new_h = d.new_h, r.new_w = d.new_w, r.nr = h, r.kv = window;
                    r.h_pass = d.new_w != w, r.v_pass = 1;
                    r.refused = MME_K1_REFUSED_TILE_TAPS;
                    out[i] = r;
                    continue;
                }
            } else {
                fit_to_canvas(h, w, &d.new_h, &d.new_w);
            }
            plan_crop(p, i, d);
            const K1Layout lay = k1_layout(d.h, d.w, d.new_h, d.new_w);
            r.new_h = d.new_h, r.new_w = d.new_w, r.nr = h;
            r.gh = lay.gh, r.kv = lay.kv;
            r.tab_off = d.tab_off, r.tmp_off = d.tmp_off;
            if (d.new_w != w) {
                tab_lds = k1_h_table_lds(w, d.new_w);
                nrows = h;
            }
        }
        r.h_pass = r.new_w != w;
        r.v_pass = r.new_h != h;
        r.tab_bytes = (int64_t)(p.tab_bytes - tab0);
        r.tmp_bytes = (int64_t)(p.tmp_bytes - tmp0);
        if (nrows > 0) {
            const BandShape b = band_shape(row_bytes, tab_lds, nrows);
            r.h_class = b.cls, r.band_rows = b.rows, r.n_bands = b.nbands;
            const size_t smem = k1_h_lds_request(b.lds);
            r.h_lds = (int32_t)smem;
            if (smem > (size_t)K1_LDS_LIMIT) r.refused = MME_K1_REFUSED_H_LDS;
        }
        if (rule.kind != MME_K1_RULE_TILES) {
            const int kvs = k1_v_stride(r.kv);
            r.v_lds = k1_v_lds_request(kvs);
            if (kvs > MAX_TAPS && !r.refused) r.refused = MME_K1_REFUSED_V_TAPS;
        }
        out[i] = r;
    }
}
