// C ABI of the device cap (include/mme.h, mme_lanczos_*): the host tables of Resample.c's LANCZOS filter, the argument
// checks and the two launches.  mme_lanczos_resize touches NO buffer of the context: scratch image and tables live in
// the caller's workspace, so calls on different workspaces never share state (the one recorded GPU fault
// was two threads in one context's scratch tables).
#include <cmath>
#include <mutex>
#include <vector>

#include "ctx.h"
#include "lanczos.h"
#include "resample.h"

namespace {

constexpr int MAX_IN = 32768, MAX_OUT = 8000, MAX_RATIO = 16;

// Resample.c precompute_coeffs: ksize of an axis (box = whole image)
int axis_ksize(int in_size, int out_size) { return resample_ksize<Lanczos3>(in_size, out_size); }

// precompute_coeffs + normalize_coeffs_8bpc for every output coordinate (resample.h): bounds(xx, xmin, n) and
// coeff(xx, i, coefficient) for i < ksize (zero from n on).  The filter values of a coordinate are kept between the
// summation and the division, so sin is called once per tap.
template <class Bounds, class Coeff>
void axis_table(int in_size, int out_size, Bounds bounds, Coeff coeff) {
    const int ksize = axis_ksize(in_size, out_size);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const Taps t = resample_taps<Lanczos3>(in_size, out_size, xx, ksize, [&](int i, int k) { coeff(xx, i, k); }, w.data());
        bounds(xx, t.xmin, t.n);
        for (int x = t.n; x < ksize; ++x) coeff(xx, x, 0);
    }
}

// The device form of an axis (lanczos.h): rows {xmin, n, k...} of `stride` ints.  An unchanged axis is not filtered:
// one-tap windows of weight 2^22 copy exactly.
void device_table(int in_size, int out_size, int stride, int32_t* t) {
    if (in_size == out_size) {
        for (int x = 0; x < out_size; ++x) {
            int32_t* row = t + (size_t)x * stride;
            row[0] = x;
            row[1] = 1;
            row[2] = 1 << PRECISION_BITS;
            for (int i = 3; i < stride; ++i) row[i] = 0;
        }
        return;
    }
    axis_table(
        in_size, out_size,
        [&](int xx, int xmin, int n) {
            t[(size_t)xx * stride] = xmin;
            t[(size_t)xx * stride + 1] = n;
        },
        [&](int xx, int i, int k) { t[(size_t)xx * stride + 2 + i] = k; });
}

int axis_stride(int in_size, int out_size) { return lz_stride(in_size == out_size ? 1 : axis_ksize(in_size, out_size)); }

std::mutex g_noctx_err;  // the context-less entries share mme_last_error(NULL)'s text
template <class... A>
int fail_noctx(const char* fmt, A... a) {
    std::lock_guard<std::mutex> lock(g_noctx_err);
    return fail(nullptr, MME_E_ARG, fmt, a...);
}

// the geometry check of all three entries; c may be null
template <class Fail>
int check_axis(Fail&& f, const char* who, const char* in_name, int in_size, const char* out_name, int out_size) {
    if (in_size < 1 || in_size > MAX_IN) return f("%s: %s = %d; supported 1..%d", who, in_name, in_size, MAX_IN);
    if (out_size < 1 || out_size > MAX_OUT) return f("%s: %s = %d; supported 1..%d (what mme_preprocess takes)", who, out_name, out_size, MAX_OUT);
    if ((int64_t)in_size > (int64_t)MAX_RATIO * out_size)
        return f("%s: %s / %s = %d / %d; supported: a ratio of at most %d (ksize <= %d)", who, in_name, out_name, in_size, out_size, MAX_RATIO,
                 LZ_MAX_KSIZE);
    return MME_OK;
}

// Image.resize (PIL/Image.py, Pillow 12) resizes an image more than 100 times as high as wide that gets lower
// vertically first, as two calls of the C resize; the intermediate image is rounded to bytes, so the order shows.
bool vertical_first(int h, int w, int new_h) { return (int64_t)h > (int64_t)w * 100 && new_h < h; }

// One launch of a pass along one axis.  The horizontal kernel reads rows at any address and pitch and writes a
// 16-byte-pitched scratch image; the vertical kernel reads such an image and writes packed rows at any address.  So the
// usual order is H (w -> new_w) | V (h -> new_h), an unchanged axis copying through one-tap windows, and the
// vertical-first order is H (copy) | V (h -> new_h) | H (w -> new_w) | V (copy): two more passes over an image that is
// at most 327 pixels wide.
struct Stage {
    bool horizontal;
    int in_size, out_size;  // the axis the pass filters
    int lines;              // H: rows of the image; V: pixels of a row
    int stride;             // of its table
    size_t tab_off, out_off;  // in the workspace; out_off of the last stage is unused (it writes dst)
};
struct Layout {  // the caller's workspace, from its first 256-byte aligned address on
    Stage st[4];
    int n;
    size_t total;
};
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
Layout layout(int h, int w, int new_h, int new_w) {
    Layout L{};
    if (vertical_first(h, w, new_h)) {
        L.n = 4;
        L.st[0] = Stage{true, w, w, h, 0, 0, 0};
        L.st[1] = Stage{false, h, new_h, w, 0, 0, 0};
        L.st[2] = Stage{true, w, new_w, new_h, 0, 0, 0};
        L.st[3] = Stage{false, new_h, new_h, new_w, 0, 0, 0};
    } else {
        L.n = 2;
        L.st[0] = Stage{true, w, new_w, h, 0, 0, 0};
        L.st[1] = Stage{false, h, new_h, new_w, 0, 0, 0};
    }
    size_t off = 0;
    for (int i = 0; i < L.n; ++i) {
        Stage& s = L.st[i];
        s.stride = axis_stride(s.in_size, s.out_size);
        s.tab_off = off;
        off += up256((size_t)s.out_size * s.stride * 4 + 16);  // + the last slice's word rounding
        if (i + 1 < L.n) {
            s.out_off = off;
            // H: lines rows of 16-byte-pitched out_size pixels + the vertical pass's over-read of its last column tile;
            // V: out_size packed rows of `lines` pixels (+ a word for the horizontal pass's aligned fetch)
            off += s.horizontal ? up256((size_t)s.lines * lz_tmp_pitch(s.out_size) + LZ_CB) : up256((size_t)s.out_size * s.lines * 3 + 16);
        }
    }
    L.total = off;
    return L;
}

// the horizontal pass's LDS plan, from the table itself: the widest window of a tile of LZ_TX columns.  Up to 96 KiB of
// LDS per workgroup: at the largest ratio the table slice is 50 KiB and a row slot 7 KiB (6 rows); ordinary caps (ratio
// < 2) run 32-row bands in under 40 KiB.
bool plan_h(const int32_t* tab, int out_size, int stride, LzPlan& p) {
    int widest = 0;
    for (int x0 = 0; x0 < out_size; x0 += LZ_TX) {
        const int x1 = (x0 + LZ_TX < out_size ? x0 + LZ_TX : out_size) - 1;
        const int lo = tab[(size_t)x0 * stride];
        const int hi = tab[(size_t)x1 * stride] + tab[(size_t)x1 * stride + 1];
        if (hi - lo > widest) widest = hi - lo;
    }
    p.slot = (15 + widest * 3 + 16 + 1023) & ~1023;
    p.tab_pad_h = (LZ_TX * stride * 4 + 1023) & ~1023;
    int rows = (96 * 1024 - p.tab_pad_h) / p.slot;
    rows = rows > LZ_H_ROWS ? LZ_H_ROWS : (rows >= 2 * LZ_H_RPT ? rows / (2 * LZ_H_RPT) * (2 * LZ_H_RPT) : rows);
    p.rows_h = rows;
    return rows >= 1;
}

}  // namespace

int mme_lanczos_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int* ksize) {
    const char* who = "mme_lanczos_tables";
    auto f = [](const char* fmt, auto... a) { return fail_noctx(fmt, a...); };
    if (int r = check_axis(f, who, "in_size", in_size, "out_size", out_size)) return r;
    if (!ksize) return fail_noctx("%s: ksize is null", who);
    if ((bounds == nullptr) != (coeffs == nullptr)) return fail_noctx("%s: bounds and coeffs must both be set or both be null", who);
    const int ks = axis_ksize(in_size, out_size);
    *ksize = ks;
    if (!bounds) return MME_OK;
    axis_table(
        in_size, out_size,
        [&](int xx, int xmin, int n) {
            bounds[2 * xx] = xmin;
            bounds[2 * xx + 1] = n;
        },
        [&](int xx, int i, int k) { coeffs[(size_t)xx * ks + i] = k; });
    return MME_OK;
}

int mme_lanczos_workspace(int h, int w, int new_h, int new_w, size_t* bytes) {
    const char* who = "mme_lanczos_workspace";
    auto f = [](const char* fmt, auto... a) { return fail_noctx(fmt, a...); };
    if (int r = check_axis(f, who, "h", h, "new_h", new_h)) return r;
    if (int r = check_axis(f, who, "w", w, "new_w", new_w)) return r;
    if (!bytes) return fail_noctx("%s: bytes is null", who);
    *bytes = layout(h, w, new_h, new_w).total + 256;  // + alignment of the caller's address
    return MME_OK;
}

int mme_lanczos_resize(mme_ctx* c, const uint8_t* src, int64_t src_pitch, int h, int w, uint8_t* dst, int new_h, int new_w, void* work,
                       size_t work_bytes, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_lanczos_resize";
    auto f = [c](const char* fmt, auto... a) { return fail(c, MME_E_ARG, fmt, a...); };
    if (int r = check_axis(f, who, "h", h, "new_h", new_h)) return r;
    if (int r = check_axis(f, who, "w", w, "new_w", new_w)) return r;
    if (src_pitch < (int64_t)3 * w) return fail(c, MME_E_ARG, "%s: src_pitch_bytes = %lld; at least 3 * w = %d is required", who, (long long)src_pitch, 3 * w);
    if (!src || !dst || !work) return fail(c, MME_E_ARG, "%s: %s is null", who, !src ? "src_dev" : (!dst ? "dst_dev" : "work_dev"));
    const Layout L = layout(h, w, new_h, new_w);
    if (work_bytes < L.total + 256)
        return fail(c, MME_E_ARG, "%s: work_bytes = %zu; mme_lanczos_workspace asks for %zu", who, work_bytes, L.total + 256);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = (uint8_t*)(((uintptr_t)work + 255) & ~(uintptr_t)255);

    // every stage's table in one host block (locals of this call: nothing is shared between threads)
    size_t ints = 0, at[4];
    for (int i = 0; i < L.n; ++i) {
        at[i] = ints;
        ints += (size_t)L.st[i].out_size * L.st[i].stride;
    }
    std::vector<int32_t> host(ints);
    LzPlan plan[4];
    for (int i = 0; i < L.n; ++i) {
        const Stage& st = L.st[i];
        device_table(st.in_size, st.out_size, st.stride, host.data() + at[i]);
        plan[i] = LzPlan{0, 0, 0, (LZ_TY * st.stride * 4 + 1023) & ~1023};
        if (st.horizontal && !plan_h(host.data() + at[i], st.out_size, st.stride, plan[i]))
            return fail(c, MME_E_STATE, "%s: no LDS plan for a %d-byte row slot beside a %d-byte table slice", who, plan[i].slot, plan[i].tab_pad_h);
    }
    for (int i = 0; i < L.n; ++i)
        HIP_TRY(c, hipMemcpyAsync(base + L.st[i].tab_off, host.data() + at[i], (size_t)L.st[i].out_size * L.st[i].stride * sizeof(int32_t),
                                  hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // `host` is a local: its staging copy must be done before it goes away
    const uint8_t* in = src;
    int64_t in_pitch = src_pitch;
    for (int i = 0; i < L.n; ++i) {
        const Stage& st = L.st[i];
        const int32_t* tab = (const int32_t*)(base + st.tab_off);
        uint8_t* out = i + 1 < L.n ? base + st.out_off : dst;
        if (st.horizontal) {
            const int pitch = lz_tmp_pitch(st.out_size);
            HIP_TRY(c, launch_lanczos_h(in, in_pitch, st.lines, st.out_size, tab, st.stride, out, pitch, plan[i], s));
            in_pitch = pitch;
        } else {
            HIP_TRY(c, launch_lanczos_v(in, (int)in_pitch, st.in_size, st.out_size, st.lines, tab, st.stride, out, plan[i], s));
            in_pitch = (int64_t)st.lines * 3;
        }
        in = out;
    }
    return MME_OK;
}
