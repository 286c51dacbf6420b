// C ABI (include/mme.h): context, K1 (preprocessing) and the launch sequences that are no encoder pass (the image towers:
// image_tower.hip; weight loading: weight_load.hip).
// No exceptions cross the boundary; every failure sets ctx->err and returns a code.
#include "../../include/mme.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "encoder_pass.h"
#include "k1_plan.h"
#include "resample.h"

namespace {

thread_local std::string g_create_error;

}  // namespace


int fail(mme_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c)
        c->err = buf;
    else
        g_create_error = buf;
    return code;
}


int ensure(mme_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return MME_OK;
    if (b.p) {
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, MME_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    b.bytes = bytes;
    return MME_OK;
}

Timed::Timed(mme_ctx* c_, hipStream_t s_, int cls) : c(c_), s(s_) {
    if (!c->prof) return;
    if (c->events_used == c->events.size()) {
        EventPair p{};
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
        c->events.push_back(p);
    }
    ev = &c->events[c->events_used++];
    ev->cls = cls;
    (void)hipEventRecord(ev->a, s);
}
Timed::~Timed() {
    if (ev) (void)hipEventRecord(ev->b, s);
}

namespace {


int set_lut(mme_ctx* c, const float mean[3], const float stdv[3]) {
    // u8 -> ((f32)(f64(u) * (1/255)) - mean) / std : transformers image_transforms.py:89-125, :384-440
    float h[768];
    for (int ch = 0; ch < 3; ++ch)
        for (int u = 0; u < 256; ++u) {
            const float x = (float)((double)u * (1.0 / 255.0));
            h[ch * 256 + u] = (x - mean[ch]) / stdv[ch];
        }
    if (!c->lut) {
        void* p = nullptr;
        HIP_TRY(c, hipMalloc(&p, sizeof h));
        c->lut = (float*)p;
    }
    HIP_TRY(c, hipMemcpy(c->lut, h, sizeof h, hipMemcpyHostToDevice));
    // The patch emitter rounds the table value to bf16.  Look for (a, b) per channel with bf16(fma(u, a, b)) == bf16(table[u])
    // for ALL 256 u: start from the f64-rounded slope / offset and try the f32 neighbours (up to 8 ulps each way, nearest
    // first, the slope in the outer loop).  The starting pair itself serves the CLIP, the ImageNet, the 0.5 / 0.5 and the
    // 0 / 1 constants; about one set in twenty needs a neighbour, and about one in a thousand has no pair on some channel
    // -- a mean within about 1e-5 of u / 255 for some u (0.6, 0.4, 0.5098) makes table[u] 0 or the few bits that the
    // cancellation in x - mean leaves, which no fma near the rounded pair gives -- and then the kernel keeps reading the table
    // for all three channels (exact = 0).
    // tests/test_gpu_normalisation.py restates this search with an exact fma, predicts the form and the pair of each of its
    // constant sets (all three kinds) and holds both emitters to the oracle bit for bit under them.
    NormAffine aff{};
    aff.exact = 1;
    for (int ch = 0; ch < 3 && aff.exact; ++ch) {
        const float a0 = (float)((1.0 / 255.0) / (double)stdv[ch]), b0 = (float)(-(double)mean[ch] / (double)stdv[ch]);
        bool found = false;
        for (int da = 0; da <= 8 && !found; ++da)
            for (int sa = -1; sa <= 1 && !found; sa += 2) {
                if (da == 0 && sa == 1) continue;
                float a = a0;
                for (int k = 0; k < da; ++k) a = std::nextafterf(a, sa < 0 ? -INFINITY : INFINITY);
                for (int db = 0; db <= 8 && !found; ++db)
                    for (int sb = -1; sb <= 1 && !found; sb += 2) {
                        if (db == 0 && sb == 1) continue;
                        float b = b0;
                        for (int k = 0; k < db; ++k) b = std::nextafterf(b, sb < 0 ? -INFINITY : INFINITY);
                        bool ok = true;
                        for (int u = 0; u < 256 && ok; ++u) ok = f32_to_bf16_rne(std::fmaf((float)u, a, b)) == f32_to_bf16_rne(h[ch * 256 + u]);
                        if (ok) {
                            aff.a[ch] = a;
                            aff.b[ch] = b;
                            found = true;
                        }
                    }
            }
        if (!found) aff.exact = 0;
    }
    c->norm_aff = aff;
    return MME_OK;
}

// copies the band lists to the device (class 0 | class 1 | class 2)
int run_h_pass(mme_ctx* c, K1Plan& p, const uint8_t* pix, int n, hipStream_t s, const char* who) {
    c->h_work.clear();
    for (int k = 0; k < 3; ++k) {
        p.count[k] = (int)p.work[k].size();
        c->h_work.insert(c->h_work.end(), p.work[k].begin(), p.work[k].end());
    }
    int r;
    if ((r = ensure(c, c->tmp, p.tmp_bytes + 16))) return r;
    if ((r = ensure(c, c->htab, p.tab_bytes + 16))) return r;
    if ((r = ensure(c, c->hwork, (c->h_work.size() + 1) * sizeof(HWork)))) return r;
    if (!c->h_work.empty())
        HIP_TRY(c, hipMemcpyAsync(c->hwork.p, c->h_work.data(), c->h_work.size() * sizeof(HWork), hipMemcpyHostToDevice, s));
    return MME_OK;
}
// the tables of every crop + the horizontal pass (one launch per class), for either descriptor: `tables` and `resize_h` are
// the rule's launchers, `rule` what the error text calls its pass
template <class Desc, class Tables, class ResizeH>
int launch_h_pass(mme_ctx* c, const K1Plan& p, const uint8_t* pix, int n, hipStream_t s, const char* who, const char* rule, Tables tables, ResizeH resize_h) {
    const Desc* crops = (const Desc*)c->crops.p;
    if (p.tab_bytes) HIP_TRY(c, tables(crops, n, (uint8_t*)c->htab.p, s));
    const HWork* work = (const HWork*)c->hwork.p;
    for (int k = 0; k < 3; ++k) {
        hipError_t e = resize_h(pix, (uint8_t*)c->tmp.p, crops, work, p.count[k], p.lds[k], k, (const uint8_t*)c->htab.p, s);
        if (e != hipSuccess) return fail(c, MME_E_HIP, "%s: %shorizontal pass, class %d (%s); %d bytes of LDS", who, rule, k, hipGetErrorString(e), p.lds[k]);
        work += p.count[k];
    }
    return MME_OK;
}
int launch_h_pass(mme_ctx* c, const K1Plan& p, const uint8_t* pix, int n, hipStream_t s, const char* who) {
    return launch_h_pass<CropDesc>(c, p, pix, n, s, who, "", launch_resample_tables, launch_resize_h);
}

// ---- K1 under MME_RESIZE_CLIP and MME_RESIZE_SPEC (preprocess_clip.hip): kClipSpec and the plan are k1_plan.h's ---------------
// the spec mme_preprocess runs under the context's rule; null under the fit-and-pad rule
const mme_resize_spec* spec_of(const mme_ctx* c) {
    return c->resize_rule == MME_RESIZE_SPEC ? &c->resize_spec : (c->resize_rule == MME_RESIZE_CLIP ? &kClipSpec : nullptr);
}

int preprocess_chunk_spec(mme_ctx* c, const mme_resize_spec& sp, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, bf16_t* patches,
                          hipStream_t s) {
    c->h_clip_crops.resize(n);
    K1Plan plan;
    const bool bilinear = sp.resample == 2;
    for (int i = 0; i < n; ++i) {
        ClipCropDesc& d = c->h_clip_crops[i];
        d.src_off = offs[i];
        d.h = hw[2 * i];
        d.w = hw[2 * i + 1];
        plan_spec_crop(plan, i, d, sp);
    }
    int r;
    if ((r = ensure(c, c->crops, (size_t)n * sizeof(ClipCropDesc)))) return r;
    HIP_TRY(c, hipMemcpyAsync(c->crops.p, c->h_clip_crops.data(), (size_t)n * sizeof(ClipCropDesc), hipMemcpyHostToDevice, s));
    if ((r = run_h_pass(c, plan, pix, n, s, "mme_preprocess"))) return r;
    Timed t(c, s, KC_PRE);
    const int resample = sp.resample;
    auto tables = [resample](const ClipCropDesc* crops, int m, uint8_t* tab, hipStream_t st) { return launch_clip_tables(crops, m, tab, resample, st); };
    if ((r = launch_h_pass<ClipCropDesc>(c, plan, pix, n, s, "mme_preprocess", bilinear ? "BILINEAR " : "BICUBIC ", tables, launch_clip_resize_h))) return r;
    HIP_TRY(c, launch_clip_v_patchify((const uint8_t*)c->tmp.p, (const ClipCropDesc*)c->crops.p, n, c->lut, c->norm_aff, patches, (const uint8_t*)c->htab.p, plan.kv_max, s));
    return MME_OK;
}

}  // namespace

int preprocess_chunk(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, bf16_t* patches, hipStream_t s) {
    c->h_crops.resize(n);
    c->h_work.clear();
    K1Plan plan;
    bool any_resize = false;
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        if (h <= 0 || w <= 0 || h > 8000 || w > 8000)
            return fail(c, MME_E_ARG, "crop %d has size %dx%d (h x w); supported 1..8000 (embedder.py:110-114 caps at 8000)", i, h, w);
        if (h != VIT_IMG || w != VIT_IMG) any_resize = true;
    }
    // a batch of 224 x 224 crops is the identity under the fit-and-pad rule and under every spec that resizes such a crop to
    // 224 x 224 (CLIP's among them): the lean instantiation below, today's bits and time.  Under any other spec (shortest
    // edge 256: resized to 256 x 256 and cropped) it is filtered like every other batch.
    if (const mme_resize_spec* sp = spec_of(c); sp && (any_resize || !spec_keeps_canvas(*sp)))
        return preprocess_chunk_spec(c, *sp, pix, offs, hw, n, patches, s);
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        CropDesc& d = c->h_crops[i];
        d.src_off = offs[i];
        d.h = h;
        d.w = w;
        fit_to_canvas(h, w, &d.new_h, &d.new_w);
        plan_crop(plan, i, d);
    }
    int r;
    if ((r = ensure(c, c->crops, (size_t)n * sizeof(CropDesc)))) return r;
    // pageable-host copies: the runtime stages them before returning, so the host vectors
    // may be reused by the next chunk
    HIP_TRY(c, hipMemcpyAsync(c->crops.p, c->h_crops.data(), (size_t)n * sizeof(CropDesc), hipMemcpyHostToDevice, s));
    if ((r = run_h_pass(c, plan, pix, n, s, "mme_preprocess"))) return r;
    Timed t(c, s, KC_PRE);
    if ((r = launch_h_pass(c, plan, pix, n, s, "mme_preprocess"))) return r;
    HIP_TRY(c, launch_resize_v_patchify(pix, (const uint8_t*)c->tmp.p, (const CropDesc*)c->crops.p, n, c->lut, c->norm_aff, patches, any_resize,
                                        (const uint8_t*)c->htab.p, plan.kv_max, s));
    return MME_OK;
}

int pool_grids_host(mme_ctx* c, const char* who, const int32_t* hw, int n, int32_t* out) {
    const int patch = c->geom.patch, g = VIT_IMG / patch;
    // every spec resizes to at least 224 on both axes and takes the centre window: the canvas is full (so is a 224 x 224 crop's,
    // which the fit-and-pad rule leaves as it is)
    const bool full = spec_of(c) != nullptr;
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        if (h <= 0 || w <= 0 || h > 8000 || w > 8000) return fail(c, MME_E_ARG, "%s: crop %d has size %dx%d (h x w); supported 1..8000", who, i, h, w);
        int nh = VIT_IMG, nw = VIT_IMG;
        if (!full) fit_to_canvas(h, w, &nh, &nw);
        out[2 * i] = full ? g : (nh + patch - 1) / patch;
        out[2 * i + 1] = full ? g : (nw + patch - 1) / patch;
    }
    return MME_OK;
}

extern "C" {

int mme_abi_version(void) { return MME_ABI_VERSION; }
int mme_is_diag_build(void) {
#ifdef MME_DIAG
    return 1;
#else
    return 0;
#endif
}

int mme_create(int device, mme_ctx** out) {
    if (!out) return fail(nullptr, MME_E_ARG, "mme_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, MME_E_HIP, "mme_create: no HIP device visible (%s)", e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(nullptr, MME_E_ARG, "mme_create: device %d out of range (0..%d)", device, count - 1);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, MME_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, MME_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MME_E_HIP, "mme_create: device %d is %s; this library carries gfx950 (MI355X) code only", device, prop.gcnArchName);
    mme_ctx* c = new (std::nothrow) mme_ctx();
    if (!c) return fail(nullptr, MME_E_NOMEM, "mme_create: out of host memory");
    c->device = device;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    int r = set_lut(c, mean, stdv);
    if (r) {
        g_create_error = c->err;
        delete c;
        return r;
    }
    *out = c;
    return MME_OK;
}

void mme_destroy(mme_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (void* p : c->allocs) (void)hipFree(p);
    DevBuf* bufs[] = {&c->x, &c->hbuf, &c->qkv, &c->att, &c->mlp, &c->patches, &c->tmp, &c->htab, &c->crops, &c->hwork, &c->page_ws, &c->cluster_ws, &c->stats, &c->lnpart, &c->neigh_ws, &c->zero_bias, &c->attn_guard, &c->attn_apply, &c->pooled, &c->projf, &c->retiled, &c->pool_grids};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (c->lut) (void)hipFree(c->lut);
    tile_vit_free(c);
    text_free(c);
    mllama_free(c);
    for (auto& ev : c->events) {
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    delete c;
}

const char* mme_last_error(const mme_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int mme_vit_geometry(mme_ctx* c, int32_t out[6]) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_vit_geometry: null argument");
    const int32_t g[6] = {VIT_IMG, c->geom.patch, c->geom.hidden, c->geom.layers, c->geom.heads, c->geom.mlp};
    for (int i = 0; i < 6; ++i) out[i] = g[i];
    return MME_OK;
}

int mme_encoder_info(mme_ctx* c, int32_t out[4]) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_encoder_info: null argument");
    out[0] = c->dinov2 ? 3 : c->siglip ? 2 : c->clip ? 1 : 0;
    out[1] = embed_dim(c);
    out[2] = c->act;
    out[3] = c->proj_dim;
    return MME_OK;
}

int mme_set_normalisation(mme_ctx* c, const float mean[3], const float stdv[3]) {
    if (!c || !mean || !stdv) return fail(c, MME_E_ARG, "mme_set_normalisation: null argument");
    for (int i = 0; i < 3; ++i)
        if (!(stdv[i] > 0.f)) return fail(c, MME_E_ARG, "mme_set_normalisation: std[%d] must be > 0", i);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    return set_lut(c, mean, stdv);
}

int mme_set_resize_rule(mme_ctx* c, int rule) {
    if (!c) return MME_E_ARG;
    if (rule != MME_RESIZE_FIT_PAD && rule != MME_RESIZE_CLIP)
        return fail(c, MME_E_ARG, "mme_set_resize_rule: rule %d; supported %d (MME_RESIZE_FIT_PAD: fit into 224 x 224, BILINEAR, zero pad) and %d "
                                  "(MME_RESIZE_CLIP: shortest edge 224, BICUBIC, centre crop); %d (MME_RESIZE_SPEC) has parameters and is set by "
                                  "mme_set_resize_spec", rule, MME_RESIZE_FIT_PAD, MME_RESIZE_CLIP, MME_RESIZE_SPEC);
    c->resize_rule = rule;
    return MME_OK;
}

int mme_set_resize_spec(mme_ctx* c, const mme_resize_spec* spec) {
    if (!c) return MME_E_ARG;
    if (!spec) return fail(c, MME_E_ARG, "mme_set_resize_spec: spec is NULL; supported: a pointer to an mme_resize_spec");
    const mme_resize_spec sp = *spec;
    const bool exact = sp.mode == MME_RESIZE_MODE_EXACT;
    if (sp.mode != MME_RESIZE_MODE_SHORTEST_EDGE && !exact)
        return fail(c, MME_E_ARG, "mme_set_resize_spec: mode = %d; supported %d (MME_RESIZE_MODE_SHORTEST_EDGE) and %d (MME_RESIZE_MODE_EXACT)", sp.mode,
                    MME_RESIZE_MODE_SHORTEST_EDGE, MME_RESIZE_MODE_EXACT);
    if (sp.height < VIT_IMG || sp.height > 512)
        return fail(c, MME_E_ARG, "mme_set_resize_spec: height = %d (%s); supported 224..512", sp.height, exact ? "the height of the resized image" : "the shortest edge");
    if (exact ? (sp.width < VIT_IMG || sp.width > 512) : sp.width != 0)
        return fail(c, MME_E_ARG, "mme_set_resize_spec: width = %d; supported %s", sp.width, exact ? "224..512" : "0 under MME_RESIZE_MODE_SHORTEST_EDGE (height is the edge)");
    if (sp.resample != 2 && sp.resample != 3)
        return fail(c, MME_E_ARG, "mme_set_resize_spec: resample = %d; supported 2 (Pillow BILINEAR) and 3 (Pillow BICUBIC)", sp.resample);
    c->resize_spec = sp;
    c->resize_rule = MME_RESIZE_SPEC;
    return MME_OK;
}

int mme_get_resize_spec(mme_ctx* c, mme_resize_spec* out) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_get_resize_spec: null argument");
    if (c->resize_rule != MME_RESIZE_SPEC)
        return fail(c, MME_E_STATE, "mme_get_resize_spec: the current rule is %d, not %d (MME_RESIZE_SPEC); mme_set_resize_spec makes a spec the rule", c->resize_rule,
                    MME_RESIZE_SPEC);
    *out = c->resize_spec;
    return MME_OK;
}

int mme_resize_rule(mme_ctx* c, int32_t* rule) {
    if (!c || !rule) return fail(c, MME_E_ARG, "mme_resize_rule: null argument");
    *rule = c->resize_rule;
    return MME_OK;
}

int mme_normalisation_form(mme_ctx* c, int32_t* exact, float a[3], float b[3]) {
    if (!c || !exact || !a || !b) return fail(c, MME_E_ARG, "mme_normalisation_form: null argument");
    *exact = c->norm_aff.exact;
    for (int i = 0; i < 3; ++i) {
        a[i] = c->norm_aff.a[i];
        b[i] = c->norm_aff.b[i];
    }
    return MME_OK;
}

int mme_set_gemm_variant(mme_ctx* c, int variant) {
    if (!c) return MME_E_ARG;
    if (variant < 0 || variant > 6) return fail(c, MME_E_ARG, "mme_set_gemm_variant: 0 (auto), 1 (128x128), 3 (256x256, 3-deep activation ring), 4 (3 with 4 of a lane's 16 stores deferred), 6 (384x256 where built, else 4); 2 means 3, 5 means 4");
    c->gemm_variant = variant;
    return MME_OK;
}

int mme_set_ln_fusion(mme_ctx* c, int mode) {
    if (!c) return MME_E_ARG;
    if (mode < 0 || mode > 2) return fail(c, MME_E_ARG, "mme_set_ln_fusion: 0 (LayerNorm kernel), 1 (folded, statistics pass over x) or 2 (folded, partial sums from the producing GEMM)");
    c->ln_mode = mode;
    return MME_OK;
}

int mme_set_attention_mode(mme_ctx* c, int mode) {
    if (!c) return MME_E_ARG;
    if (mode < 0 || mode > 2) return fail(c, MME_E_ARG, "mme_set_attention_mode: 0 (exact row maximum), 1 (fast form, guarded; the default) or 2 (fast form with the guard forced: every launch is redone exactly)");
    c->attn_mode = mode;
    return MME_OK;
}

int mme_attention_redone(mme_ctx* c, int32_t flags[12]) {
    if (!c || !flags) return fail(c, MME_E_ARG, "mme_attention_redone: null argument");
    const int nl = c->geom.layers < 12 ? c->geom.layers : 12;  // the first min(12, layers) words; mme_attention_redone_n for more
    for (int l = 0; l < nl; ++l) flags[l] = 0;
    if (!c->attn_guard.p) return MME_OK;  // no pass has run yet
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(flags, c->attn_guard.p, nl * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MME_OK;
}

int mme_attention_redone_n(mme_ctx* c, int count, int32_t* flags) {
    if (!c || !flags) return fail(c, MME_E_ARG, "mme_attention_redone_n: null argument");
    if (count < 1 || count > 64) return fail(c, MME_E_ARG, "mme_attention_redone_n: count %d outside 1..64", count);
    for (int l = 0; l < count; ++l) flags[l] = 0;
    if (!c->attn_guard.p) return MME_OK;  // no pass has run yet
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(flags, c->attn_guard.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MME_OK;
}

int mme_attention_apply(mme_ctx* c, int kind, const uint16_t* qkv, int n, const int32_t* ntiles_host, int only_block, int reverse,
                        uint16_t* out, int32_t* redone, void* stream) {
    if (!c) return MME_E_ARG;
    if (!qkv || !out || !redone) return fail(c, MME_E_ARG, "mme_attention_apply: null argument");
    if (kind != 0 && kind != 1) return fail(c, MME_E_ARG, "mme_attention_apply: kind %d (0 = ViT/16 at the context's geometry, 1 = tile-ViT)", kind);
    const TokenLayout& L = c->geom.layout();
    if (kind == 0 && L.attn != ATTN_LONG)
        return fail(c, MME_E_ARG, "mme_attention_apply: kind 0 is the 197-token kernel and the context holds a patch-%d tower (%d tokens); %s op 2 launches its kernel", L.patch, L.tokens, L.patch == 32 ? "mme_vit32_apply" : "mme_dinov2_apply");
    const int n_max = kind == 0 ? 1 << 20 : 4096;
    if (n <= 0 || n > n_max) return fail(c, MME_E_ARG, "mme_attention_apply: n = %d outside 1..%d", n, n_max);
    if (kind == 0) {
        if (!L.takes_block(only_block)) return fail(c, MME_E_ARG, "mme_attention_apply: only_block %d outside -1..%d", only_block, L.blocks - 1);
        if (reverse != 0 && reverse != 1) return fail(c, MME_E_ARG, "mme_attention_apply: reverse must be 0 or 1");
    } else {
        if (only_block != -1 || reverse != 0) return fail(c, MME_E_ARG, "mme_attention_apply: kind 1 takes only_block = -1 and reverse = 0");
        if (!ntiles_host) return fail(c, MME_E_ARG, "mme_attention_apply: kind 1 needs ntiles_host");
        for (int i = 0; i < n; ++i)
            if (ntiles_host[i] < 1 || ntiles_host[i] > 4) return fail(c, MME_E_ARG, "mme_attention_apply: image %d uses %d tiles (1..4)", i, ntiles_host[i]);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure(c, c->attn_apply, (16 + (size_t)n) * sizeof(int32_t)))) return r;
    hipStream_t s = (hipStream_t)stream;
    int* guard = (int*)c->attn_apply.p;
    int32_t* nt_dev = (int32_t*)c->attn_apply.p + 16;
    HIP_TRY(c, hipMemsetAsync(guard, 0, sizeof(int), s));
    if (kind == 0) {
        HIP_TRY(c, launch_attention(qkv, out, n, c->geom.heads, s, c->attn_mode ? guard : nullptr, c->attn_mode == 2, only_block, reverse != 0, c->geom.tokens()));
    } else {
        HIP_TRY(c, hipMemcpyAsync(nt_dev, ntiles_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(c, launch_attention_tiles(qkv, out, nt_dev, n, s, c->attn_mode ? guard : nullptr, c->attn_mode == 2));
    }
    int32_t g = 0;
    HIP_TRY(c, hipMemcpyAsync(&g, guard, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    *redone = g != 0;
    return MME_OK;
}

int mme_set_tile_order(mme_ctx* c, int mode) {
    if (!c) return MME_E_ARG;
    if (mode < 0 || mode > 2) return fail(c, MME_E_ARG, "mme_set_tile_order: 0 (every kernel walks the rows upwards), 1 (zig-zag, the default) or 2 (only the attention walks downwards)");
    c->zigzag = mode;
    return MME_OK;
}

int mme_set_forward_pruning(mme_ctx* c, int on) {
    if (!c) return MME_E_ARG;
    c->prune_last = on != 0;
    return MME_OK;
}

// ---- pooling over the covered patch tokens -------------------------------------------------------------------
int mme_set_pooling(mme_ctx* c, int mode) {
    if (!c) return MME_E_ARG;
    if (mode < MME_POOL_TOKEN || mode > MME_POOL_CLS_MEAN)
        return fail(c, MME_E_ARG, "mme_set_pooling: mode = %d; supported %d (MME_POOL_TOKEN), %d (MME_POOL_MEAN) and %d (MME_POOL_CLS_MEAN)", mode, MME_POOL_TOKEN,
                    MME_POOL_MEAN, MME_POOL_CLS_MEAN);
    if (mode != MME_POOL_TOKEN) {
        const char* enc = !c->loaded ? (c->tv ? "tile_vit" : "none loaded") : c->siglip ? "siglip" : c->clip ? "clip" : nullptr;
        if (enc)
            return fail(c, MME_E_STATE, "mme_set_pooling: mode = %d with encoder %s; supported: modes %d and %d with a vit or dinov2 tower loaded (CLIP's "
                                        "projection and SigLIP's head pool for themselves), mode %d everywhere", mode, enc, MME_POOL_MEAN, MME_POOL_CLS_MEAN, MME_POOL_TOKEN);
    }
    c->pool_mode = mode;
    return MME_OK;
}

int mme_pooling(mme_ctx* c, int32_t* mode) {
    if (!c || !mode) return fail(c, MME_E_ARG, "mme_pooling: null argument");
    *mode = c->pool_mode;
    return MME_OK;
}

int mme_pool_grid(int h, int w, int patch, int32_t out_rc[2]) {
    if (!out_rc) return fail(nullptr, MME_E_ARG, "mme_pool_grid: out_rc is NULL");
    if (h < 1 || h > 8000 || w < 1 || w > 8000) return fail(nullptr, MME_E_ARG, "mme_pool_grid: crop size %dx%d (h x w); supported 1..8000", h, w);
    if (patch != 14 && patch != 16 && patch != 32) return fail(nullptr, MME_E_ARG, "mme_pool_grid: patch = %d; supported 14, 16 and 32", patch);
    int nh, nw;
    fit_to_canvas(h, w, &nh, &nw);
    out_rc[0] = (nh + patch - 1) / patch;  // a patch counts when it holds at least one pixel of the resized crop
    out_rc[1] = (nw + patch - 1) / patch;
    return MME_OK;
}

int mme_k1_plan(const mme_k1_rule* rule, const int32_t* hw, int n, mme_k1_record* out, int64_t totals[4], int32_t* bands, int64_t bands_cap) {
    if (!rule || n < 0 || (n > 0 && (!hw || !out))) return fail(nullptr, MME_E_ARG, "mme_k1_plan: null argument or n < 0");
    if (rule->kind < MME_K1_RULE_FIT_PAD || rule->kind > MME_K1_RULE_TILES)
        return fail(nullptr, MME_E_ARG, "mme_k1_plan: rule kind = %d; supported 0 (fit-and-pad), 1 (resize spec) and 2 (tiles)", rule->kind);
    if (rule->kind == MME_K1_RULE_SPEC && !spec_admitted(rule->spec))
        return fail(nullptr, MME_E_ARG, "mme_k1_plan: spec {mode %d, height %d, width %d, resample %d} is none mme_set_resize_spec admits", rule->spec.mode,
                    rule->spec.height, rule->spec.width, rule->spec.resample);
    if (rule->kind == MME_K1_RULE_TILES && !tiles_admitted(rule->tile, rule->max_tiles))
        return fail(nullptr, MME_E_ARG, "mme_k1_plan: need tile in 8..1024 (multiple of 8), max_tiles in 1..16; got %d, %d", rule->tile, rule->max_tiles);
    K1Plan plan;
    plan.list_bands = bands != nullptr;
    k1_plan_records(*rule, hw, n, out, plan);
    if (totals) {
        totals[0] = (int64_t)plan.tab_bytes;
        totals[1] = (int64_t)plan.tmp_bytes;
        totals[2] = (int64_t)plan.nbands;
        totals[3] = plan.kv_max;
    }
    if (bands) {
        if ((int64_t)plan.nbands > bands_cap)
            return fail(nullptr, MME_E_ARG, "mme_k1_plan: the batch has %zu bands, bands_host holds %lld", plan.nbands, (long long)bands_cap);
        for (int k = 0; k < 3; ++k)  // the order run_h_pass copies them in
            for (const HWork& wk : plan.work[k]) {
                *bands++ = wk.crop;
                *bands++ = wk.row0;
                *bands++ = wk.nrows;
                *bands++ = k;
            }
    }
    return MME_OK;
}

int mme_pool_grids(mme_ctx* c, const int32_t* hw, int n, int32_t* grids) {
    if (!c) return MME_E_ARG;
    if (n < 0 || (n > 0 && (!hw || !grids))) return fail(c, MME_E_ARG, "mme_pool_grids: null argument or n<0");
    return pool_grids_host(c, "mme_pool_grids", hw, n, grids);
}

int mme_pool_apply(mme_ctx* c, int op, const mme_pool_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_pool_apply", a, op, 1)) return r;
    const HookCheck h{c, "mme_pool_apply", op};
    if (int r = h.width(a->d)) return r;
    if (int r = h.ln_in(a->x, a->gamma, a->beta)) return r;
    if (int r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16")) return r;
    if (a->grids && ((uintptr_t)a->grids & 7) != 0) return h.needs("grids 8-byte aligned (device int32 [B, 2]) or NULL");
    if (a->B < 0 || a->B > (1 << 20)) return fail(c, MME_E_ARG, "mme_pool_apply: B = %d outside 0..2^20", a->B);
    if (a->g < 1 || a->g > 16) return fail(c, MME_E_ARG, "mme_pool_apply: g = %d; supported 1..16", a->g);
    if (a->first != 0 && a->first != 1) return fail(c, MME_E_ARG, "mme_pool_apply: first = %d; supported 0 and 1", a->first);
    if (op == 1 && a->first != 1) return fail(c, MME_E_ARG, "mme_pool_apply: op 1 (cls+mean) needs first == 1: row 0 is the class row (first = %d)", a->first);
    if (a->tokens != a->first + a->g * a->g)
        return fail(c, MME_E_ARG, "mme_pool_apply: tokens = %d; supported first + g * g = %d", a->tokens, a->first + a->g * a->g);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(c, launch_pool_mean(a->x, a->gamma, a->beta, a->grids, a->B, a->tokens, a->g, a->first, op == 1, a->d, a->eps, a->emb_f32, a->emb_bf16, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

int mme_set_chunk(mme_ctx* c, int crops) {
    if (!c) return MME_E_ARG;
    if (crops < 1 || crops > 16384) return fail(c, MME_E_ARG, "mme_set_chunk: %d outside 1..16384", crops);
    c->chunk = crops;
    return MME_OK;
}

int mme_normalise_rows(mme_ctx* c, const float* x, int64_t rows, int d, uint16_t* y, void* stream) {
    if (!c) return MME_E_ARG;
    if (rows < 0 || d <= 0 || (d % 4) != 0) return fail(c, MME_E_ARG, "mme_normalise_rows: rows >= 0 and d %% 4 == 0 required");
    if (rows == 0) return MME_OK;
    if (!x || !y) return fail(c, MME_E_ARG, "mme_normalise_rows: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    Timed t(c, (hipStream_t)stream, KC_POOL);
    HIP_TRY(c, launch_normalise_rows(x, rows, d, y, (hipStream_t)stream));
    return MME_OK;
}

int mme_cosine(mme_ctx* c, const uint16_t* a, int m, const uint16_t* b, int n, int d, float* sim, int64_t ld, void* stream) {
    if (!c) return MME_E_ARG;
    if (m < 0 || n < 0 || d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "mme_cosine: m,n >= 0 and d %% 64 == 0 required (d=%d)", d);
    if (m == 0 || n == 0) return MME_OK;
    if (!a || !b || !sim || ld < n) return fail(c, MME_E_ARG, "mme_cosine: null pointer or ld_sim < n");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    Timed t(c, s, KC_COS);
    GemmArgs g{};
    g.A = a; g.W = b; g.M = m; g.N = n; g.K = d; g.outf = sim; g.ldf = ld;
    HIP_TRY(c, launch_gemm(EPI_F32, g, s, c->gemm_variant));
    return MME_OK;
}

int mme_cosine_bf16(mme_ctx* c, const uint16_t* a, int m, const uint16_t* b, int n, int d, uint16_t* sim, int64_t ld, void* stream) {
    if (!c) return MME_E_ARG;
    if (m < 0 || n < 0 || d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "mme_cosine_bf16: m,n >= 0 and d %% 64 == 0 required (d=%d)", d);
    if (m == 0 || n == 0) return MME_OK;
    if (!a || !b || !sim || ld < n || (ld % 8) != 0 || (n % 4) != 0)
        return fail(c, MME_E_ARG, "mme_cosine_bf16: null pointer, ld_sim < n, ld_sim %% 8 != 0 or n %% 4 != 0");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the bf16 epilogues add a bias vector: a resident row of zeros (acc + 0.0f is exact), grown on demand
    if (c->zero_bias.bytes < (size_t)n * sizeof(float)) {
        int r = ensure(c, c->zero_bias, ((size_t)n * sizeof(float) + 4095) & ~(size_t)4095);
        if (r) return r;
        HIP_TRY(c, hipMemsetAsync(c->zero_bias.p, 0, c->zero_bias.bytes, s));
    }
    Timed t(c, s, KC_COS);
    GemmArgs g{};
    g.A = a; g.W = b; g.M = m; g.N = n; g.K = d; g.bias = (const float*)c->zero_bias.p; g.out = sim; g.ldo = ld;
    HIP_TRY(c, launch_gemm(EPI_BIAS, g, s, c->gemm_variant));
    return MME_OK;
}

static int page_similarity_impl(mme_ctx* c, const uint16_t* emb, int64_t N, int d, const double* area_pct, const uint8_t* valid,
                                const int32_t* page_offs_host, int P, const uint8_t* skip, int max_query, int top_k, double max_dist,
                                int metric, int normalise, int64_t pair_lo, int64_t pair_hi, double* S, void* stream) {
    if (!c) return MME_E_ARG;
    if (P < 0 || N < 0 || d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "mme_page_similarity: bad sizes (P=%d N=%lld d=%d)", P, (long long)N, d);
    if (P == 0) return MME_OK;
    if (!S || !page_offs_host) return fail(c, MME_E_ARG, "mme_page_similarity: null pointer");
    if (N > 0 && (!emb || !area_pct || !valid)) return fail(c, MME_E_ARG, "mme_page_similarity: null pointer");
    if (max_query < 1 || top_k < 1 || max_query * top_k > 128) return fail(c, MME_E_ARG, "mme_page_similarity: max_query*top_k must be in 1..128");
    if (metric != 0 && metric != 1) return fail(c, MME_E_ARG, "mme_page_similarity: metric must be 0 (cosine) or 1 (sqeuclidean)");
    if (page_offs_host[0] != 0 || page_offs_host[P] != N) return fail(c, MME_E_ARG, "mme_page_similarity: page_offs must run 0..N");
    for (int p = 0; p < P; ++p)
        if (page_offs_host[p + 1] < page_offs_host[p]) return fail(c, MME_E_ARG, "mme_page_similarity: page_offs not monotone at %d", p);
    if (N >= (int64_t)1 << 31) return fail(c, MME_E_ARG, "mme_page_similarity: N too large");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t slots = (size_t)P * max_query;
    // workspace carve: page_offs | qrow | nvalid | maxbuf | qemb | qsim
    size_t o_offs = 0;
    size_t o_qrow = o_offs + (((size_t)(P + 1) * 4 + 255) & ~(size_t)255);
    size_t o_nval = o_qrow + ((slots * 4 + 255) & ~(size_t)255);
    size_t o_max = o_nval + (((size_t)P * 4 + 255) & ~(size_t)255);
    size_t o_qemb = o_max + 256;
    size_t o_qsim = o_qemb + ((slots * d * 2 + 255) & ~(size_t)255);
    size_t total = o_qsim + slots * (size_t)(N > 0 ? N : 1) * 4;
    int r = ensure(c, c->page_ws, total);
    if (r) return r;
    char* ws = (char*)c->page_ws.p;
    HIP_TRY(c, hipMemcpyAsync(ws + o_offs, page_offs_host, (size_t)(P + 1) * 4, hipMemcpyHostToDevice, s));
    Timed t(c, s, KC_PAGE);
    PageSimArgs a{};
    a.emb = emb; a.N = N; a.d = d; a.area_pct = area_pct; a.valid = valid;
    a.page_offs = (const int32_t*)(ws + o_offs); a.P = P; a.skip = skip;
    a.max_query = max_query; a.top_k = top_k; a.max_dist = max_dist; a.metric = metric; a.normalise = normalise;
    a.pair_lo = pair_lo; a.pair_hi = pair_hi;
    a.S = S; a.qsim = (float*)(ws + o_qsim); a.qrow = (const int32_t*)(ws + o_qrow); a.qpage = (const int32_t*)(ws + o_nval);
    a.qstart = nullptr; a.nq = (int)slots; a.qemb = ws + o_qemb; a.maxbuf = (double*)(ws + o_max);
    HIP_TRY(c, launch_page_similarity(a, s));
    return MME_OK;
}

int mme_page_similarity(mme_ctx* c, const uint16_t* emb, int64_t N, int d, const double* area_pct, const uint8_t* valid,
                        const int32_t* page_offs_host, int P, const uint8_t* skip, int max_query, int top_k, double max_dist,
                        int metric, int normalise, double* S, void* stream) {
    return page_similarity_impl(c, emb, N, d, area_pct, valid, page_offs_host, P, skip, max_query, top_k, max_dist, metric, normalise, 0, -1,
                                S, stream);
}

int mme_page_similarity_pairs(mme_ctx* c, const uint16_t* emb, int64_t N, int d, const double* area_pct, const uint8_t* valid,
                              const int32_t* page_offs_host, int P, const uint8_t* skip, int max_query, int top_k, double max_dist,
                              int metric, int64_t pair_lo, int64_t pair_hi, double* S, void* stream) {
    if (c && (pair_lo < 0 || pair_hi < pair_lo || pair_hi > (int64_t)P * (P - 1) / 2))
        return fail(c, MME_E_ARG, "mme_page_similarity_pairs: pair range [%lld, %lld) outside 0..P(P-1)/2", (long long)pair_lo, (long long)pair_hi);
    return page_similarity_impl(c, emb, N, d, area_pct, valid, page_offs_host, P, skip, max_query, top_k, max_dist, metric, 0, pair_lo, pair_hi,
                                S, stream);
}

int mme_cluster_pages(mme_ctx* c, const double* S, int P, int n_clusters, int mode, int32_t* labels, int32_t* k_out, double* scores,
                      void* stream) {
    if (!c) return MME_E_ARG;
    if (!S || !labels || !k_out || !scores) return fail(c, MME_E_ARG, "mme_cluster_pages: null pointer");
    if (P < 2 || P > 4096) return fail(c, MME_E_ARG, "mme_cluster_pages: P=%d outside 2..4096", P);
    if (n_clusters < 0 || n_clusters > P) return fail(c, MME_E_ARG, "mme_cluster_pages: n_clusters=%d outside 0..P", n_clusters);
    if (mode != 0 && mode != 1) return fail(c, MME_E_ARG, "mme_cluster_pages: mode must be 0 (reference fallback) or 1 (precomputed)");
    HIP_TRY(c, hipSetDevice(c->device));
    int r = ensure(c, c->cluster_ws, cluster_workspace_bytes(P));
    if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, hipMemsetAsync(scores, 0xff, 16 * sizeof(double), s));  // NaN = "not evaluated"
    HIP_TRY(c, launch_cluster(S, P, n_clusters, mode, (char*)c->cluster_ws.p, labels, k_out, scores, s));
    return MME_OK;
}

// ---- Mllama tile canvas: the grid and the fit are k1_plan.h's ----
int mme_preprocess_tiles(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, int tile, int max_tiles,
                         float* out, int32_t* aspect_ids_host, int32_t* num_tiles_host, void* stream) {
    if (!c) return MME_E_ARG;
    if (n < 0 || !tiles_admitted(tile, max_tiles))
        return fail(c, MME_E_ARG, "mme_preprocess_tiles: need n >= 0, tile in 8..1024 (multiple of 8), max_tiles in 1..16");
    if (n == 0) return MME_OK;
    if (!pix || !offs || !hw || !out) return fail(c, MME_E_ARG, "mme_preprocess_tiles: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->h_crops.resize(n);
    c->h_work.clear();
    std::vector<int32_t> grid((size_t)n * 2);
    K1Plan plan;
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        if (h <= 0 || w <= 0 || h > 8000 || w > 8000) return fail(c, MME_E_ARG, "crop %d has size %dx%d (h x w); supported 1..8000", i, h, w);
        CropDesc& d = c->h_crops[i];
        d.src_off = offs[i];
        d.h = h;
        d.w = w;
        int th, tw;
        if (const int window = tile_crop_size(d, tile, max_tiles, &th, &tw))
            return fail(c, MME_E_ARG, "mme_preprocess_tiles: crop %d is %dx%d (h x w) and becomes %d rows: a vertical window of %d taps; the limit is %d taps",
                        i, h, w, d.new_h, window, MAX_TAPS);
        grid[2 * i] = th;
        grid[2 * i + 1] = tw;
        if (aspect_ids_host) {  // 1 + index of (th, tw) in the supported list (image_processing_pil_mllama.py:136-164)
            int idx = 0, found = 0;
            for (int a = 1; a <= max_tiles && !found; ++a)
                for (int b = 1; b <= max_tiles; ++b) {
                    if (a * b > max_tiles) continue;
                    ++idx;
                    if (a == th && b == tw) { found = idx; break; }
                }
            aspect_ids_host[i] = found;
        }
        if (num_tiles_host) num_tiles_host[i] = th * tw;
        plan_crop(plan, i, d);
    }
    int r;
    const size_t desc_bytes = ((size_t)n * sizeof(CropDesc) + 15) & ~(size_t)15;
    if ((r = ensure(c, c->crops, desc_bytes + grid.size() * sizeof(int32_t)))) return r;
    HIP_TRY(c, hipMemcpyAsync(c->crops.p, c->h_crops.data(), (size_t)n * sizeof(CropDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync((char*)c->crops.p + desc_bytes, grid.data(), grid.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if ((r = run_h_pass(c, plan, pix, n, s, "mme_preprocess_tiles"))) return r;
    HIP_TRY(c, hipStreamSynchronize(s));  // `grid` is a local: its staging copy must be done before it goes away
    Timed t(c, s, KC_PRE);
    if ((r = launch_h_pass(c, plan, pix, n, s, "mme_preprocess_tiles"))) return r;
    HIP_TRY(c, launch_resize_v_tiles(pix, (const uint8_t*)c->tmp.p, (const CropDesc*)c->crops.p, (const int32_t*)((char*)c->crops.p + desc_bytes),
                                     n, c->lut, out, tile, max_tiles, s));
    return MME_OK;
}

int mme_crop_boxes(mme_ctx* c, const uint8_t* page, int H, int W, const int32_t* boxes, int n, uint8_t* pix, const int64_t* offs,
                   void* stream) {
    if (!c) return MME_E_ARG;
    if (n < 0 || H <= 0 || W <= 0) return fail(c, MME_E_ARG, "mme_crop_boxes: bad sizes (n=%d, page %dx%d)", n, H, W);
    if (n == 0) return MME_OK;
    if (!page || !boxes || !pix || !offs) return fail(c, MME_E_ARG, "mme_crop_boxes: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    c->h_work.clear();
    for (int i = 0; i < n; ++i) {
        // corners are any int32: x1 - x0 of two of them needs 33 bits
        const int64_t w64 = (int64_t)boxes[4 * i + 2] - boxes[4 * i], h64 = (int64_t)boxes[4 * i + 3] - boxes[4 * i + 1];
        if (w64 <= 0 || h64 <= 0 || w64 > 8000 || h64 > 8000)
            return fail(c, MME_E_ARG, "mme_crop_boxes: box %d is %lldx%lld (w x h); supported 1..8000", i, (long long)w64, (long long)h64);
        const int w = (int)w64, h = (int)h64;
        int rows = (32 * 1024) / (w * 3);
        rows = rows < 1 ? 1 : rows;
        for (int r = 0; r < h; r += rows) c->h_work.push_back(HWork{i, r, (h - r) < rows ? (h - r) : rows});
    }
    int r;
    const size_t bbytes = (size_t)n * 4 * sizeof(int32_t), obytes = (size_t)n * sizeof(int64_t);
    if ((r = ensure(c, c->hwork, (c->h_work.size() + 1) * sizeof(HWork)))) return r;
    if ((r = ensure(c, c->crops, bbytes + obytes + 16))) return r;
    char* meta = (char*)c->crops.p;  // offs (8-byte aligned) | boxes
    HIP_TRY(c, hipMemcpyAsync(meta, offs, obytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(meta + obytes, boxes, bbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->hwork.p, c->h_work.data(), c->h_work.size() * sizeof(HWork), hipMemcpyHostToDevice, s));
    Timed t(c, s, KC_PRE);
    HIP_TRY(c, launch_crop_boxes(page, H, W, (const int32_t*)(meta + obytes), (const int64_t*)meta, (const HWork*)c->hwork.p,
                                 (int)c->h_work.size(), pix, s));
    return MME_OK;
}

int mme_nms_boxes(mme_ctx* c, const double* boxes, const double* scores, const int32_t* classes, const int32_t* page_offs, int pages,
                  double iou_threshold, int32_t* keep, int32_t* keep_count, void* stream) {
    if (!c) return MME_E_ARG;
    if (pages < 0) return fail(c, MME_E_ARG, "mme_nms_boxes: pages = %d", pages);
    if (pages == 0) return MME_OK;
    if (!page_offs || !keep_count) return fail(c, MME_E_ARG, "mme_nms_boxes: null pointer");
    if (page_offs[0] != 0) return fail(c, MME_E_ARG, "mme_nms_boxes: page_offs[0] must be 0");
    for (int p = 0; p < pages; ++p) {
        const int64_t k = (int64_t)page_offs[p + 1] - page_offs[p];
        if (k < 0 || k > 32768) return fail(c, MME_E_ARG, "mme_nms_boxes: page %d has %lld boxes; supported 0..32768 per page", p, (long long)k);
    }
    const size_t n = (size_t)page_offs[pages];
    if (n && (!boxes || !scores || !classes || !keep)) return fail(c, MME_E_ARG, "mme_nms_boxes: null pointer");
    if (!(iou_threshold == iou_threshold)) return fail(c, MME_E_ARG, "mme_nms_boxes: iou_threshold is NaN");
    // a NaN score has no place in "the highest-scoring box that is left" (3_combine_grids.py:104: max() / list.index
    // on a NaN depend on where it sits in the list); json.load accepts NaN, so say so instead of ranking garbage
    for (size_t i = 0; i < n; ++i)
        if (!(scores[i] == scores[i])) return fail(c, MME_E_ARG, "mme_nms_boxes: scores[%zu] is NaN", i);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // one staging block: boxes | scores | classes | order | keep | page_offs | keep_count
    const size_t o_sc = n * 32, o_cl = o_sc + n * 8, o_or = o_cl + n * 4, o_kp = o_or + n * 4, o_po = (o_kp + n * 4 + 15) & ~(size_t)15;
    const size_t o_kc = o_po + ((size_t)(pages + 1) * 4 + 15) / 16 * 16, total = o_kc + (size_t)pages * 4 + 16;
    int r;
    if ((r = ensure(c, c->hwork, total))) return r;
    char* d = (char*)c->hwork.p;
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(d, boxes, n * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(d + o_sc, scores, n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(d + o_cl, classes, n * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemcpyAsync(d + o_po, page_offs, (size_t)(pages + 1) * 4, hipMemcpyHostToDevice, s));
    {
        Timed t(c, s, KC_PRE);
        HIP_TRY(c, launch_nms_pages((const double*)d, (const double*)(d + o_sc), (const int32_t*)(d + o_cl), (const int32_t*)(d + o_po), pages,
                                    iou_threshold, (int32_t*)(d + o_or), (int32_t*)(d + o_kp), (int32_t*)(d + o_kc), s));
    }
    if (n) HIP_TRY(c, hipMemcpyAsync(keep, d + o_kp, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(keep_count, d + o_kc, (size_t)pages * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // results are host data (the JSON of the next step is built from them)
    return MME_OK;
}

int mme_neighbours(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, int row0, int nrows, int fetch, int top_n,
                   int keep_self, float min_sim, float max_sim, int32_t* idx, float* sim, void* stream) {
    if (!c) return MME_E_ARG;
    if (N < 0 || nrows < 0 || row0 < 0 || d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "mme_neighbours: bad sizes (N=%d nrows=%d d=%d)", N, nrows, d);
    if (fetch < 1 || fetch > 128 || top_n < 1 || top_n > 128) return fail(c, MME_E_ARG, "mme_neighbours: fetch and top_n must be in 1..128");
    if (nrows == 0) return MME_OK;
    if ((int64_t)row0 + nrows > N) return fail(c, MME_E_ARG, "mme_neighbours: query rows [%d, %d) exceed N=%d", row0, row0 + nrows, N);
    if (!emb || !idx || !sim) return fail(c, MME_E_ARG, "mme_neighbours: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // cosine block of a chunk of query rows: [rc, ldq] f32, at most 2 GiB (the top-k runs one wave per row and
    // needs thousands of rows to fill the chip: 64 MiB chunks ran 6x slower), whole 256-row GEMM tiles
    const int64_t ldq = ((int64_t)N + 3) & ~(int64_t)3;
    static const int64_t ws_mb = getenv("MME_NEIGH_WS_MB") ? atoll(getenv("MME_NEIGH_WS_MB")) : 2048;
    int64_t rc = (ws_mb << 20) / (ldq * 4);
    rc = rc < 256 ? 256 : (rc / 256) * 256;
    if (rc > nrows) rc = nrows;
    const int nchunks = (int)((nrows + rc - 1) / rc);

    // Fused form (large N): the cosine block is never written.  (1) a strided sample of the rows (every 8th)
    // gives, per query, a lower bound tau on its fetch-th best similarity; (2) the full GEMM runs with the
    // EPI_TOPK epilogue, which appends every (value >= tau, column) to the query's candidate list instead of
    // storing the tile; (3) the same streaming selection runs over the short lists.  A full list (clustered
    // data beating the 4x margin) raises a device flag that arms an unfused re-run of that chunk -- decided
    // on the device, so the call stays asynchronous and the result exact either way.
    constexpr int kStride = 8;
    const int ns = N / kStride;
    const int64_t tiles256 = ((int64_t)(rc + 255) / 256) * ((N + 255) / 256);
    const bool fused = c->neigh_mode != 1 && d >= 128 && ns >= 2048 && ns >= fetch && tiles256 >= 256 && (c->neigh_mode == 2 || N >= 16384);
    if (c->neigh_mode == 2 && !fused)
        return fail(c, MME_E_ARG, "mme_neighbours: the fused form needs N >= 16384 rows and >= 256 cosine tiles per chunk (N=%d, rows=%d)", N, nrows);
    const int64_t ldqs = ((int64_t)ns + 3) & ~(int64_t)3;
    int64_t cap = 32 * (int64_t)fetch;
    cap = cap < 256 ? 256 : (cap > 8192 ? 8192 : cap);
    size_t o_qsim = 0, o_samp = 0, o_qs = 0, o_tidx = 0, o_tsim = 0, o_cnt = 0, o_flag = 0, o_cval = 0, o_cidx = 0, total = (size_t)rc * ldq * 4;
    if (fused) {
        auto carve = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) & ~(size_t)255; return o; };
        o_samp = carve((size_t)ns * d * 2);
        o_qs = carve((size_t)rc * ldqs * 4);
        o_tidx = carve((size_t)rc * fetch * 4);
        o_tsim = carve((size_t)rc * fetch * 4);
        o_cnt = carve((size_t)rc * 4);
        o_flag = carve((size_t)nchunks * 4);
        o_cval = carve((size_t)rc * cap * 4);
        o_cidx = carve((size_t)rc * cap * 4);
    }
    int r;
    if ((r = ensure(c, c->neigh_ws, total))) return r;
    char* ws = (char*)c->neigh_ws.p;
    float* qsim = (float*)(ws + o_qsim);
    Timed t(c, s, KC_NEIGH);
    if (fused) {
        HIP_TRY(c, hipMemcpy2DAsync(ws + o_samp, (size_t)d * 2, emb, (size_t)kStride * d * 2, (size_t)d * 2, ns, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemsetAsync(ws + o_flag, 0, (size_t)nchunks * 4, s));
    }
    for (int64_t c0 = 0; c0 < nrows; c0 += rc) {
        const int m = (int)(nrows - c0 < rc ? nrows - c0 : rc);
        const int q0 = (int)(row0 + c0);
        int32_t* idx_o = idx + (size_t)c0 * top_n;
        float* sim_o = sim + (size_t)c0 * top_n;
        GemmArgs g{};
        g.A = emb + (size_t)q0 * d; g.W = emb; g.M = m; g.N = N; g.K = d; g.outf = qsim; g.ldf = ldq;
        if (!fused) {
            HIP_TRY(c, launch_gemm(EPI_F32, g, s, c->gemm_variant));
            HIP_TRY(c, launch_topk_rows(qsim, ldq, N, m, q0, group, fetch, top_n, keep_self, min_sim, max_sim, idx_o, sim_o, s));
            continue;
        }
        int* flag = (int*)(ws + o_flag) + (int)(c0 / rc);
        float* tsim = (float*)(ws + o_tsim);
        // (1) thresholds from the sample: fetch-th best of [m, ns]
        GemmArgs gs = g;
        gs.W = ws + o_samp; gs.N = ns; gs.outf = (float*)(ws + o_qs); gs.ldf = ldqs;
        HIP_TRY(c, launch_gemm(EPI_F32, gs, s, c->gemm_variant));
        HIP_TRY(c, launch_topk_rows((const float*)(ws + o_qs), ldqs, ns, m, 0, nullptr, fetch, fetch, 1, -INFINITY, INFINITY,
                                    (int32_t*)(ws + o_tidx), tsim, s));
        // (2) full GEMM, candidates only
        HIP_TRY(c, hipMemsetAsync(ws + o_cnt, 0, (size_t)m * 4, s));
        GemmArgs gf = g;
        gf.outf = nullptr; gf.thr = tsim + (fetch - 1); gf.thr_stride = fetch; gf.cand_count = (int*)(ws + o_cnt);
        gf.cand_val = (float*)(ws + o_cval); gf.cand_idx = (int*)(ws + o_cidx); gf.cand_cap = (int)cap; gf.overflow = flag;
        HIP_TRY(c, launch_gemm(EPI_TOPK, gf, s, 3));
        // (3) exact selection over the candidate lists
        HIP_TRY(c, launch_topk_candidates(gf.cand_val, gf.cand_idx, gf.cand_count, (int)cap, m, q0, group, fetch, top_n, keep_self, min_sim,
                                          max_sim, idx_o, sim_o, s));
        // fallback, armed on the device by an overflowing list
        g.run_if = flag;
        HIP_TRY(c, launch_gemm(EPI_F32, g, s, 3));
        HIP_TRY(c, launch_topk_rows(qsim, ldq, N, m, q0, group, fetch, top_n, keep_self, min_sim, max_sim, idx_o, sim_o, s, flag));
    }
    return MME_OK;
}

int mme_set_neighbour_mode(mme_ctx* c, int mode) {
    if (!c) return MME_E_ARG;
    if (mode < 0 || mode > 2) return fail(c, MME_E_ARG, "mme_set_neighbour_mode: 0 (by size), 1 (cosine block through the workspace) or 2 (fused candidate lists)");
    c->neigh_mode = mode;
    return MME_OK;
}

static int gemm_bench_impl(mme_ctx* c, int M, int N, int K, int epilogue, int variant, int iters, double* avg_ms, uint64_t* stamps_host) {
    if (!c || !avg_ms) return MME_E_ARG;
    if (M <= 0 || N <= 0 || K <= 0 || (K % 64) != 0 || (N % 4) != 0 || iters < 1 || epilogue < 0 || epilogue > 4)
        return fail(c, MME_E_ARG, "mme_gemm_bench: bad shape / epilogue");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t a_bytes = (size_t)M * K * 2, w_bytes = (size_t)N * K * 2, o_bytes = (size_t)(M + 256) * N * 4;
    void *A = nullptr, *W = nullptr, *O = nullptr, *B = nullptr, *P = nullptr, *ST = nullptr;
    constexpr size_t kStampBytes = 256 * 2 * 16 * sizeof(uint64_t);
    std::vector<uint16_t> h(((a_bytes > w_bytes ? a_bytes : w_bytes) / 2));
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto fill = [&](size_t n) {  // uniform [-1,1) bf16 (guide: bench on random data, never zeros)
        for (size_t i = 0; i < n; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const float f = (float)((int64_t)(x >> 40) - (1 << 23)) * (1.0f / (1 << 23));
            h[i] = f32_to_bf16_rne(f);
        }
    };
    int rc = MME_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    do {
        if (hipMalloc(&A, a_bytes) != hipSuccess || hipMalloc(&W, w_bytes) != hipSuccess || hipMalloc(&O, o_bytes) != hipSuccess ||
            hipMalloc(&B, (size_t)N * 4) != hipSuccess || hipMalloc(&P, (size_t)VIT_T * N * 4) != hipSuccess) { rc = fail(c, MME_E_NOMEM, "mme_gemm_bench: hipMalloc"); break; }
        fill(a_bytes / 2);
        if (hipMemcpy(A, h.data(), a_bytes, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(c, MME_E_HIP, "memcpy"); break; }
        fill(w_bytes / 2);
        if (hipMemcpy(W, h.data(), w_bytes, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(c, MME_E_HIP, "memcpy"); break; }
        (void)hipMemset(O, 0, o_bytes); (void)hipMemset(B, 0, (size_t)N * 4); (void)hipMemset(P, 0, (size_t)VIT_T * N * 4);
        GemmArgs g{};
        g.A = A; g.W = W; g.M = M; g.N = N; g.K = K; g.bias = (const float*)B; g.out = O; g.ldo = N; g.res = O; g.pos = (const float*)P;
        g.outf = (float*)O; g.ldf = N;
        if (epilogue == EPI_PATCH) g.M = (M / VIT_NP) * VIT_NP;
        hipStream_t s = nullptr;
        hipError_t e = launch_gemm(epilogue, g, s, variant);  // warm-up
        if (e != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_gemm_bench launch: %s", hipGetErrorString(e)); break; }
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; ++i) (void)launch_gemm(epilogue, g, s, variant);
        (void)hipEventRecord(e1, s);
        if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_gemm_bench: kernel failed: %s", hipGetErrorString(hipGetLastError())); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *avg_ms = ms / iters;
        if (stamps_host) {
            if (hipMalloc(&ST, kStampBytes) != hipSuccess) { rc = fail(c, MME_E_NOMEM, "mme_gemm_stamps: hipMalloc"); break; }
            (void)hipMemset(ST, 0, kStampBytes);
            (void)launch_gemm256r_stamped(g, (unsigned long long*)ST, s);  // warm
            (void)hipMemset(ST, 0, kStampBytes);
            hipError_t es = launch_gemm256r_stamped(g, (unsigned long long*)ST, s);
            if (es != hipSuccess || hipDeviceSynchronize() != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_gemm_stamps: launch failed"); break; }
            (void)hipMemcpy(stamps_host, ST, kStampBytes, hipMemcpyDeviceToHost);
        }
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (void* p : {A, W, O, B, P, ST}) if (p) (void)hipFree(p);
    return rc;
}

int mme_gemm_bench(mme_ctx* c, int M, int N, int K, int epilogue, int variant, int iters, double* avg_ms) {
    return gemm_bench_impl(c, M, N, K, epilogue, variant, iters, avg_ms, nullptr);
}

int mme_gemm_stamps(mme_ctx* c, int M, int N, int K, uint64_t* stamps_host) {
    if (!stamps_host) return MME_E_ARG;
    double ms = 0;
    // ~0.5 s of back-to-back launches of the product kernel first: the clock stamps ([13], [14]) are only
    // meaningful once DVFS has settled under this load
    return gemm_bench_impl(c, M, N, K, EPI_BIAS, 3, 150, &ms, stamps_host);
}

// ---- single launches on caller-owned operands (tests/test_gpu_gemm.py): every assumption of the kernels is checked here,
// so that a bad argument is an MME_E_ARG and never a launch
static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int mme_gemm_apply(mme_ctx* c, const mme_gemm_apply_args* a, int32_t* ran_256, void* stream) {
    if (!c) return MME_E_ARG;
    if (!a || !ran_256) return fail(c, MME_E_ARG, "mme_gemm_apply: null argument");
    const int epi = a->epilogue;
    if (epi == EPI_TOPK) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue 7 (candidate lists) is not served here; mme_select_apply op 2 launches it");
    if (epi < 0 || epi > EPI_BIAS_RES_STATS) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue %d outside 0..6, 8", epi);
    if (a->variant < 0 || a->variant > 6) return fail(c, MME_E_ARG, "mme_gemm_apply: variant %d outside 0..6", a->variant);
    if (a->reverse_m != 0 && a->reverse_m != 1) return fail(c, MME_E_ARG, "mme_gemm_apply: reverse_m must be 0 or 1");
    const int64_t M = a->M, N = a->N, K = a->K;
    if (M < 1 || M > (1 << 24) || N < 1 || N > (1 << 20)) return fail(c, MME_E_ARG, "mme_gemm_apply: M = %d outside 1..2^24 or N = %d outside 1..2^20", a->M, a->N);
    if (K < 64 || K > (1 << 16) || (K % 64) != 0) return fail(c, MME_E_ARG, "mme_gemm_apply: K = %d must be a multiple of 64 in 64..65536", a->K);
    if (!a->A || !a->W) return fail(c, MME_E_ARG, "mme_gemm_apply: null operand (A or W)");
    if (!aligned_to(a->A, 16) || !aligned_to(a->W, 16)) return fail(c, MME_E_ARG, "mme_gemm_apply: A and W must be 16-byte aligned");
    const bool patch = epi == EPI_PATCH, res = epi == EPI_BIAS_RES || epi == EPI_BIAS_RES_STATS;
    const bool ln = epi == EPI_LN_BIAS || epi == EPI_LN_BIAS_GELU;
    if (patch && (M % VIT_NP) != 0) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue 3 needs M %% %d == 0 (M = %d)", VIT_NP, a->M);
    const int64_t out_rows = patch ? M / VIT_NP * VIT_T : M;
    if (epi == EPI_F32) {
        if (!a->outf) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue 4 needs outf");
        if (a->ldf < N || a->ldf > (1 << 24)) return fail(c, MME_E_ARG, "mme_gemm_apply: ldf = %lld outside N..2^24", (long long)a->ldf);
        if (!aligned_to(a->outf, (a->ldf % 4) == 0 ? 16 : 4))
            return fail(c, MME_E_ARG, "mme_gemm_apply: outf must be 16-byte aligned when ldf %% 4 == 0 (4-byte otherwise)");
    } else {
        if ((N % 4) != 0) return fail(c, MME_E_ARG, "mme_gemm_apply: a bf16 output needs N %% 4 == 0 (N = %d)", a->N);
        if (!a->bias || !a->out) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue %d needs bias and out", epi);
        if (!aligned_to(a->bias, 16) || !aligned_to(a->out, 16)) return fail(c, MME_E_ARG, "mme_gemm_apply: bias and out must be 16-byte aligned");
        if (a->ldo < N || a->ldo > (1 << 24) || (a->ldo % 8) != 0) return fail(c, MME_E_ARG, "mme_gemm_apply: ldo = %lld must be a multiple of 8 in N..2^24", (long long)a->ldo);
    }
    if (res) {
        if (!a->res) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue %d needs res", epi);
        if (!aligned_to(a->res, 16)) return fail(c, MME_E_ARG, "mme_gemm_apply: res must be 16-byte aligned");
        const uintptr_t o0 = (uintptr_t)a->out, r0 = (uintptr_t)a->res, span = (uintptr_t)(((out_rows - 1) * a->ldo + N) * 2);
        if (r0 != o0 && r0 < o0 + span && o0 < r0 + span) return fail(c, MME_E_ARG, "mme_gemm_apply: res must be out itself or not overlap it");
    }
    if (patch) {
        if (!a->pos) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue 3 needs pos");
        if (!aligned_to(a->pos, 16)) return fail(c, MME_E_ARG, "mme_gemm_apply: pos must be 16-byte aligned");
        if (a->pos_rows < VIT_T) return fail(c, MME_E_ARG, "mme_gemm_apply: pos must hold [%d, N] (pos_rows = %lld)", VIT_T, (long long)a->pos_rows);
    }
    if (ln) {
        if (!a->ln_stats || !a->colsum) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue %d needs ln_stats and colsum", epi);
        if (!aligned_to(a->ln_stats, 8) || !aligned_to(a->colsum, 16)) return fail(c, MME_E_ARG, "mme_gemm_apply: ln_stats must be 8-byte and colsum 16-byte aligned");
    }
    const bool planes = epi == EPI_BIAS_RES_STATS || (patch && a->ln_part);
    if (planes) {
        if (!a->ln_part) return fail(c, MME_E_ARG, "mme_gemm_apply: epilogue 8 needs ln_part");
        if (!aligned_to(a->ln_part, 4)) return fail(c, MME_E_ARG, "mme_gemm_apply: ln_part must be 4-byte aligned");
        if ((N % 64) != 0) return fail(c, MME_E_ARG, "mme_gemm_apply: partial-sum planes need N %% 64 == 0 (N = %d)", a->N);
        if (a->ln_part_rows < out_rows) return fail(c, MME_E_ARG, "mme_gemm_apply: ln_part_rows = %lld is below the %lld output rows", (long long)a->ln_part_rows, (long long)out_rows);
        if (a->ln_part_rows > ((int64_t)1 << 32) || a->ln_part_floats < 2 * (N / 64) * a->ln_part_rows)
            return fail(c, MME_E_ARG, "mme_gemm_apply: ln_part holds %lld floats, [2][%lld][%lld] needs %lld", (long long)a->ln_part_floats, (long long)(N / 64),
                        (long long)a->ln_part_rows, (long long)(2 * (N / 64) * a->ln_part_rows));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = a->A; g.W = a->W; g.M = a->M; g.N = a->N; g.K = a->K;
    g.reverse_m = a->reverse_m;
    if (epi == EPI_F32) {
        g.outf = a->outf; g.ldf = a->ldf;
    } else {
        g.bias = a->bias; g.out = a->out; g.ldo = a->ldo;
    }
    if (res) g.res = a->res;
    if (patch) g.pos = a->pos;
    if (ln) { g.ln_stats = a->ln_stats; g.colsum = a->colsum; }
    if (planes) { g.ln_part = a->ln_part; g.ln_part_rows = a->ln_part_rows; }
    hipStream_t s = (hipStream_t)stream;
    *ran_256 = gemm_runs_256(g, a->variant) ? 1 : 0;
    HIP_TRY(c, launch_gemm(epi, g, s, a->variant));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

int mme_rowop_apply(mme_ctx* c, int op, const mme_rowop_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_rowop_apply", a, op, 5)) return r;
    const bool fixed_d = op == 0 || op == 1 || op == 4 || op == 5;
    if (fixed_d && !vit_width_built(a->d)) return fail(c, MME_E_ARG, "mme_rowop_apply: op %d is built for d == 384, d == 768 and d == 1024 (d = %d)", op, a->d);
    if (!fixed_d && (a->d <= 0 || (a->d % 64) != 0 || a->d > 2048)) return fail(c, MME_E_ARG, "mme_rowop_apply: op %d needs d %% 64 == 0, d <= 2048 (d = %d)", op, a->d);
    const bool stats_ok = a->stats && aligned_to(a->stats, 8);
    const char* bad = nullptr;
    const HookCheck h{c, "mme_rowop_apply", op};
    switch (op) {
        case 0:
            if (!vec16(a->x) || !vec16(a->y) || !vec16(a->gamma) || !vec16(a->beta)) bad = "x, y, gamma, beta non-null and 16-byte aligned";
            else if (a->rows < 0) bad = "rows >= 0";
            break;
        case 1:
            if (!vec16(a->x) || !stats_ok) bad = "x non-null and 16-byte aligned, stats non-null and 8-byte aligned";
            else if (a->rows < 0) bad = "rows >= 0";
            break;
        case 2:
            if (!vec16(a->x) || !stats_ok) bad = "x non-null and 16-byte aligned, stats non-null and 8-byte aligned";
            else if (a->row0 < 0 || a->row1 < a->row0 || a->stride < 1) bad = "0 <= row0 <= row1 and stride >= 1";
            break;
        case 3:
            if (!a->part || !aligned_to(a->part, 4) || !stats_ok) bad = "part non-null and 4-byte aligned, stats non-null and 8-byte aligned";
            else if (a->rows < 0 || a->rows > a->part_rows) bad = "0 <= rows <= part_rows";
            else if (a->part_rows > ((int64_t)1 << 32) || a->part_floats < 2 * (int64_t)(a->d / 64) * a->part_rows) bad = "part_floats >= 2 * d/64 * part_rows";
            break;
        case 4:
            if (!vec16(a->x) || !vec16(a->cls) || !vec16(a->pos)) bad = "x, cls, pos non-null and 16-byte aligned";
            else if (a->B < 0) bad = "B >= 0";
            break;
        default:
            if (int r = h.ln_in(a->x, a->gamma, a->beta)) return r;
            if (int r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16")) return r;
            if (a->B < 0) bad = "B >= 0";
            else if (int r = h.tok(*find_layout(VIT_T), a->tok)) return r;
            break;
    }
    if (bad) return fail(c, MME_E_ARG, "mme_rowop_apply: op %d needs %s", op, bad);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    switch (op) {
        case 0: HIP_TRY(c, launch_layernorm(a->x, a->gamma, a->beta, a->y, a->rows, a->d, a->eps, s)); break;
        case 1: HIP_TRY(c, launch_ln_stats(a->x, a->rows, a->d, a->eps, a->stats, s)); break;
        case 2: HIP_TRY(c, launch_ln_stats_canonical(a->x, a->row0, a->row1, a->d, a->eps, a->stats, s, a->stride)); break;
        case 3: HIP_TRY(c, launch_ln_finish(a->part, a->part_rows, a->rows, a->d, a->eps, a->stats, s)); break;
        case 4: HIP_TRY(c, launch_cls_rows(a->x, a->cls, a->pos, a->B, a->d, s)); break;
        default: HIP_TRY(c, launch_pool(a->x, a->gamma, a->beta, a->B, VIT_T, a->tok, a->d, a->eps, a->emb_f32, a->emb_bf16, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// the three launches of K12 (mme_neighbours), one at a time on caller-owned buffers (tests/test_gpu_select.py)
int mme_select_apply(mme_ctx* c, int op, const mme_select_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_select_apply", a, op, 2)) return r;
    auto word = [](const void* p) { return p && aligned_to(p, 4); };
    if (op <= 1) {
        if (a->nrows < 0 || a->nrows > (1 << 24)) return fail(c, MME_E_ARG, "mme_select_apply: nrows = %d outside 0..2^24", a->nrows);
        if (a->row0 < 0) return fail(c, MME_E_ARG, "mme_select_apply: row0 = %d is negative", a->row0);
        if (a->fetch < 1 || a->fetch > 128) return fail(c, MME_E_ARG, "mme_select_apply: fetch = %d outside 1..128", a->fetch);
        if (a->top_n < 1 || a->top_n > 128) return fail(c, MME_E_ARG, "mme_select_apply: top_n = %d outside 1..128", a->top_n);
        if (!word(a->idx_out) || !word(a->sim_out)) return fail(c, MME_E_ARG, "mme_select_apply: op %d needs idx_out and sim_out non-null and 4-byte aligned", op);
        if (a->group && !aligned_to(a->group, 4)) return fail(c, MME_E_ARG, "mme_select_apply: group must be 4-byte aligned");
    }
    if (op == 0) {
        if (a->N < 1) return fail(c, MME_E_ARG, "mme_select_apply: op 0 needs N >= 1 (N = %d)", a->N);
        if ((a->ld % 4) != 0 || a->ld < a->N || a->ld > ((int64_t)1 << 30))
            return fail(c, MME_E_ARG, "mme_select_apply: op 0 needs ld %% 4 == 0 and N <= ld <= 2^30 (ld = %lld, N = %d)", (long long)a->ld, a->N);
        if (!vec16(a->qsim)) return fail(c, MME_E_ARG, "mme_select_apply: op 0 needs qsim non-null and 16-byte aligned");
        if (a->run_if && !aligned_to(a->run_if, 4)) return fail(c, MME_E_ARG, "mme_select_apply: run_if must be 4-byte aligned");
    } else if (op == 1) {
        if (a->cap < 4 || (a->cap % 4) != 0) return fail(c, MME_E_ARG, "mme_select_apply: op 1 needs cap %% 4 == 0 and cap >= 4 (cap = %d)", a->cap);
        if (!vec16(a->cand_val) || !vec16(a->cand_idx) || !word(a->len))
            return fail(c, MME_E_ARG, "mme_select_apply: op 1 needs cand_val and cand_idx non-null and 16-byte aligned, len non-null and 4-byte aligned");
    } else {
        if (a->M < 0 || a->M > (1 << 24)) return fail(c, MME_E_ARG, "mme_select_apply: M = %d outside 0..2^24", a->M);
        if (a->N < 1 || a->N > (1 << 20)) return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs N in 1..2^20 (N = %d)", a->N);
        if (a->K < 128 || a->K > (1 << 16) || (a->K % 64) != 0)
            return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs K a multiple of 64 in 128..65536 (K = %d)", a->K);
        if (a->cap < 1) return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs cap >= 1 (cap = %d)", a->cap);
        if (a->thr_stride < 1) return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs thr_stride >= 1 (thr_stride = %d)", a->thr_stride);
        if (!vec16(a->A) || !vec16(a->W)) return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs A and W non-null and 16-byte aligned");
        if (!word(a->thr) || !word(a->cand_count) || !word(a->cand_val) || !word(a->cand_idx) || !word(a->overflow))
            return fail(c, MME_E_ARG, "mme_select_apply: op 2 needs thr, cand_count, cand_val, cand_idx and overflow non-null and 4-byte aligned");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (op == 0) {
        HIP_TRY(c, launch_topk_rows(a->qsim, a->ld, a->N, a->nrows, a->row0, a->group, a->fetch, a->top_n, a->keep_self, a->min_sim, a->max_sim,
                                    a->idx_out, a->sim_out, s, a->run_if));
    } else if (op == 1) {
        HIP_TRY(c, launch_topk_candidates(a->cand_val, a->cand_idx, a->len, a->cap, a->nrows, a->row0, a->group, a->fetch, a->top_n, a->keep_self,
                                          a->min_sim, a->max_sim, a->idx_out, a->sim_out, s));
    } else {
        GemmArgs g{};
        g.A = a->A; g.W = a->W; g.M = a->M; g.N = a->N; g.K = a->K;
        g.thr = a->thr; g.thr_stride = a->thr_stride; g.cand_count = a->cand_count; g.cand_val = a->cand_val; g.cand_idx = a->cand_idx;
        g.cand_cap = a->cap; g.overflow = a->overflow;
        HIP_TRY(c, launch_gemm(EPI_TOPK, g, s, 3));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// ops 0 / 1 of mme_clip_apply and mme_siglip_apply: one GEMM whose epilogue applies the tower's activation, `epi` without
// (op 0) or behind (op 1) the folded LayerNorm; the checks of mme_gemm_apply's epilogues 1 / 6 under the caller's name
static int act_gemm_apply(mme_ctx* c, const char* who, int op, int epi, const mme_gemm_apply_args* ga, int32_t* ran_256, hipStream_t s) {
    if (!ga) return fail(c, MME_E_ARG, "%s: op %d needs gemm", who, op);
    if (ga->variant < 0 || ga->variant > 6) return fail(c, MME_E_ARG, "%s: variant %d outside 0..6", who, ga->variant);
    if (ga->reverse_m != 0 && ga->reverse_m != 1) return fail(c, MME_E_ARG, "%s: reverse_m must be 0 or 1", who);
    const int64_t M = ga->M, N = ga->N, K = ga->K;
    if (M < 1 || M > (1 << 24) || N < 1 || N > (1 << 20)) return fail(c, MME_E_ARG, "%s: M = %d outside 1..2^24 or N = %d outside 1..2^20", who, ga->M, ga->N);
    if (K < 64 || K > (1 << 16) || (K % 64) != 0) return fail(c, MME_E_ARG, "%s: K = %d must be a multiple of 64 in 64..65536", who, ga->K);
    if (!ga->A || !ga->W) return fail(c, MME_E_ARG, "%s: null operand (A or W)", who);
    if (!aligned_to(ga->A, 16) || !aligned_to(ga->W, 16)) return fail(c, MME_E_ARG, "%s: A and W must be 16-byte aligned", who);
    if ((N % 4) != 0) return fail(c, MME_E_ARG, "%s: a bf16 output needs N %% 4 == 0 (N = %d)", who, ga->N);
    if (!ga->bias || !ga->out) return fail(c, MME_E_ARG, "%s: op %d needs bias and out", who, op);
    if (!aligned_to(ga->bias, 16) || !aligned_to(ga->out, 16)) return fail(c, MME_E_ARG, "%s: bias and out must be 16-byte aligned", who);
    if (ga->ldo < N || ga->ldo > (1 << 24) || (ga->ldo % 8) != 0) return fail(c, MME_E_ARG, "%s: ldo = %lld must be a multiple of 8 in N..2^24", who, (long long)ga->ldo);
    if (op == 1) {
        if (!ga->ln_stats || !ga->colsum) return fail(c, MME_E_ARG, "%s: op 1 needs ln_stats and colsum", who);
        if (!aligned_to(ga->ln_stats, 8) || !aligned_to(ga->colsum, 16)) return fail(c, MME_E_ARG, "%s: ln_stats must be 8-byte and colsum 16-byte aligned", who);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = ga->A; g.W = ga->W; g.M = ga->M; g.N = ga->N; g.K = ga->K;
    g.reverse_m = ga->reverse_m;
    g.bias = ga->bias; g.out = ga->out; g.ldo = ga->ldo;
    if (op == 1) { g.ln_stats = ga->ln_stats; g.colsum = ga->colsum; }
    if (ran_256) *ran_256 = gemm_runs_256(g, ga->variant) ? 1 : 0;
    HIP_TRY(c, launch_gemm(epi, g, s, ga->variant));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// the kernels a CLIP tower adds, one launch each (tests/test_gpu_clip.py)
int mme_clip_apply(mme_ctx* c, int op, const mme_clip_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_clip_apply", a, op, 4)) return r;
    hipStream_t s = (hipStream_t)stream;
    if (op <= 1) return act_gemm_apply(c, "mme_clip_apply", op, op == 0 ? EPI_BIAS_QGELU : EPI_LN_BIAS_QGELU, a->gemm, a->ran_256, s);
    const HookCheck h{c, "mme_clip_apply", op};
    const char* bad = nullptr;
    int r;
    if (op == 2 || op == 3) {
        if ((r = h.width(a->d)) || (r = h.ln_in(a->x, a->gamma, a->beta))) return r;
        if (op == 2 && (!a->stats || !aligned_to(a->stats, 8))) bad = "stats non-null and 8-byte aligned";
        else if (op == 2 && a->rows < 0) bad = "rows >= 0";
        else if (op == 3 && !vec16(a->y)) bad = "y non-null and 16-byte aligned";
        else if (op == 3 && a->B < 0) bad = "B >= 0";
        else if (op == 3 && (r = h.tok(*find_layout(VIT_T), a->tok))) return r;
    } else {
        if (a->p < 64 || (a->p % 64) != 0 || a->p > 1024) return fail(c, MME_E_ARG, "mme_clip_apply: op 4 needs p %% 64 == 0, 64 <= p <= 1024 (p = %d)", a->p);
        if (!vec16(a->xf)) bad = "xf non-null and 16-byte aligned";
        else if ((r = h.out_pair(a->y_f32, a->y_bf16, "y_f32", "y_bf16"))) return r;
        else if (a->rows < 0) bad = "rows >= 0";
    }
    if (bad) return h.needs(bad);
    HIP_TRY(c, hipSetDevice(c->device));
    switch (op) {
        case 2: HIP_TRY(c, launch_pre_ln(a->x, a->gamma, a->beta, a->rows, a->d, a->eps, a->stats, s)); break;
        case 3: HIP_TRY(c, launch_pool_ln(a->x, a->gamma, a->beta, a->B, VIT_T, a->tok, a->d, a->eps, a->y, s)); break;
        default: HIP_TRY(c, launch_l2_rows(a->xf, a->rows, a->p, a->y_f32, a->y_bf16, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // extern "C"

// The four steps a patch tower outside the 197-token path adds -- retile, embed rows, exact attention, the pooled
// LayerNorm without (y) or with (emb_f32 / emb_bf16) the L2 step -- one launch each at layout L: the ops mme_vit32_apply and
// mme_dinov2_apply have in common.  A is either hook's args struct; y is passed beside it (DINOv2 has no such op).
enum PatchStep { STEP_RETILE, STEP_EMBED_ROWS, STEP_ATTENTION, STEP_POOL_LN, STEP_POOL_LN_L2 };
template <class A>
static int patch_tower_apply(mme_ctx* c, const char* who, const TokenLayout& L, int op, PatchStep step, const A* a, uint16_t* y, const char* retile_how,
                             void* stream) {
    const HookCheck h{c, who, op};
    int r = h.crops(a->n);
    if (r) return r;
    switch (step) {
        case STEP_RETILE:  // retile_how: the kernel's kind of copy ("permutation", "gather")
            if (!vec16(a->src) || !vec16(a->dst)) return h.needs("src and dst non-null and 16-byte aligned");
            if ((const void*)a->src == (const void*)a->dst) return fail(c, MME_E_ARG, "%s: op %d needs src != dst (the %s is not in place)", who, op, retile_how);
            break;
        case STEP_EMBED_ROWS: r = h.embed_rows(L, a->d, a->acc, a->bias, a->pos, a->cls, a->x); break;
        case STEP_ATTENTION:
            if ((r = h.heads(L, a->heads))) return r;
            if (!vec16(a->qkv) || !vec16(a->out)) return h.needs("qkv and out non-null and 16-byte aligned");
            if (!L.takes_block(a->only_block)) return fail(c, MME_E_ARG, "%s: op %d needs only_block in -1..%d", who, op, L.blocks - 1);
            break;
        default:
            if ((r = h.width(a->d)) || (r = h.ln_in(a->x, a->gamma, a->beta)) || (r = h.tok(L, a->tok))) return r;
            if (step == STEP_POOL_LN) r = vec16(y) ? MME_OK : h.needs("y non-null and 16-byte aligned");
            else r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16");
            break;
    }
    if (r) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    switch (step) {
        case STEP_RETILE: HIP_TRY(c, launch_retile(L.patch, a->src, a->dst, a->n, s)); break;
        case STEP_EMBED_ROWS: HIP_TRY(c, launch_embed_rows(a->acc, a->bias, a->pos, a->cls, a->x, a->n, L.tokens, a->d, s)); break;
        case STEP_ATTENTION: HIP_TRY(c, launch_attention_exact(a->qkv, a->out, a->n, L.tokens, L.causal, a->heads, s, a->only_block)); break;
        case STEP_POOL_LN: HIP_TRY(c, launch_pool_ln(a->x, a->gamma, a->beta, a->n, L.tokens, a->tok, a->d, a->eps, y, s)); break;
        default: HIP_TRY(c, launch_pool(a->x, a->gamma, a->beta, a->n, L.tokens, a->tok, a->d, a->eps, a->emb_f32, a->emb_bf16, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

extern "C" {

// the kernels a patch-32 tower adds, one launch each (tests/test_gpu_vit32.py): the op codes are the steps
int mme_vit32_apply(mme_ctx* c, int op, const mme_vit32_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_vit32_apply", a, op, 4)) return r;
    return patch_tower_apply(c, "mme_vit32_apply", *find_layout(50), op, (PatchStep)op, a, a->y, "permutation", stream);
}

// the kernels a DINOv2 tower (patch 14, 257 tokens) adds, one launch each (tests/test_gpu_dinov2.py): ops 0..2 are the steps,
// op 3 the pooled LayerNorm with the L2 step; rowscale and mul (ops 4, 5) are the loader's own
int mme_dinov2_apply(mme_ctx* c, int op, const mme_dinov2_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_dinov2_apply", a, op, 5)) return r;
    if (op <= 3) return patch_tower_apply(c, "mme_dinov2_apply", *find_layout(257), op, op == 3 ? STEP_POOL_LN_L2 : (PatchStep)op, a, nullptr, "gather", stream);
    if (a->dtype < MME_DT_F32 || a->dtype > MME_DT_F16)
        return fail(c, MME_E_ARG, "mme_dinov2_apply: dtype %d (MME_DT_F32 = 0, MME_DT_BF16 = 1, MME_DT_F16 = 2)", a->dtype);
    const size_t esz = a->dtype == MME_DT_F32 ? 4 : 2;
    const char* bad = nullptr;
    if (!a->w || !a->factor || !a->prepared || ((uintptr_t)a->factor % esz)) bad = "w, factor, prepared non-null, factor aligned to its element";
    else if (a->rows < 1 || a->rows > ((int64_t)1 << 24)) bad = "1 <= rows <= 2^24";
    else if (op == 4 && (!vec16(a->w) || !vec16(a->prepared))) bad = "w and prepared 16-byte aligned";
    else if (op == 4 && (a->cols < 8 || (a->cols % 8) != 0 || a->cols > (1 << 16))) bad = "cols a multiple of 8 in 8..65536";
    else if (op == 5 && (((uintptr_t)a->w % esz) || !aligned_to(a->prepared, 4))) bad = "w aligned to its element, prepared 4-byte aligned";
    if (bad) return fail(c, MME_E_ARG, "mme_dinov2_apply: op %d needs %s", op, bad);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (op == 4) HIP_TRY(c, launch_wp_rowscale(a->dtype, a->w, (size_t)a->rows, (size_t)a->cols, a->factor, a->prepared, s));
    else HIP_TRY(c, launch_wp_mul(a->dtype, a->w, a->factor, (size_t)a->rows, (float*)a->prepared, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// the kernels a SigLIP tower adds, one launch each (tests/test_gpu_siglip.py)
int mme_siglip_apply(mme_ctx* c, int op, const mme_siglip_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_siglip_apply", a, op, 4)) return r;
    hipStream_t s = (hipStream_t)stream;
    if (op <= 1) return act_gemm_apply(c, "mme_siglip_apply", op, op == 0 ? EPI_BIAS_TGELU : EPI_LN_BIAS_TGELU, a->gemm, a->ran_256, s);
    const HookCheck h{c, "mme_siglip_apply", op};
    const TokenLayout& L = *find_layout(196);
    int r;
    if ((r = h.crops(a->n))) return r;
    if (op == 3) {
        if ((r = h.heads(L, a->heads))) return r;
        if (!vec16(a->kv) || !vec16(a->q) || !vec16(a->out)) return h.needs("kv, q and out non-null and 16-byte aligned");
    } else if (op == 2) {
        if ((r = h.embed_rows(L, a->d, a->acc, a->bias, a->pos, nullptr, a->x))) return r;
    } else {
        if ((r = h.width(a->d))) return r;
        if (!vec16(a->x)) return h.needs("x non-null and 16-byte aligned");
        if ((r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16"))) return r;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    switch (op) {
        case 2: HIP_TRY(c, launch_embed_rows(a->acc, a->bias, a->pos, nullptr, a->x, a->n, L.tokens, a->d, s)); break;
        case 3: HIP_TRY(c, launch_map_pool(a->kv, a->q, a->out, a->n, a->heads, s)); break;
        default: HIP_TRY(c, launch_l2_rows_bf16(a->x, a->n, a->d, a->emb_f32, a->emb_bf16, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// ---- the one collective (RCCL over xGMI) -------------------------------------------------------------------
#define RCCL_TRY(c, expr)                                                                           \
    do {                                                                                            \
        const int e_ = (expr);                                                                      \
        if (e_ != 0) return fail((c), MME_E_COMM, "%s: %s", #expr, rccl_error_string(e_));          \
    } while (0)

int mme_comm_unique_id(mme_ctx* c, uint8_t id[MME_COMM_ID_BYTES]) {
    if (!c || !id) return fail(c, MME_E_ARG, "mme_comm_unique_id: null argument");
    if (const char* why = rccl_ready()) return fail(c, MME_E_COMM, "%s", why);
    RCCL_TRY(c, rccl_unique_id(id));
    return MME_OK;
}

int mme_comm_init(mme_ctx* c, const uint8_t id[MME_COMM_ID_BYTES], int rank, int world, void** comm) {
    if (!c || !id || !comm) return fail(c, MME_E_ARG, "mme_comm_init: null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(c, MME_E_ARG, "mme_comm_init: rank %d outside 0..%d", rank, world - 1);
    if (const char* why = rccl_ready()) return fail(c, MME_E_COMM, "%s", why);
    HIP_TRY(c, hipSetDevice(c->device));
    *comm = nullptr;
    RCCL_TRY(c, rccl_comm_init(comm, world, id, rank));
    return MME_OK;
}

int mme_comm_destroy(mme_ctx* c, void* comm) {
    if (!c) return MME_E_ARG;
    if (!comm) return MME_OK;
    if (const char* why = rccl_ready()) return fail(c, MME_E_COMM, "%s", why);
    HIP_TRY(c, hipSetDevice(c->device));
    RCCL_TRY(c, rccl_comm_destroy(comm));
    return MME_OK;
}

int mme_allgather(mme_ctx* c, void* comm, const uint16_t* shard, int64_t rows, int d, uint16_t* all, void* stream) {
    if (!c) return MME_E_ARG;
    if (!comm || rows < 0 || d <= 0) return fail(c, MME_E_ARG, "mme_allgather: null communicator or bad sizes (rows=%lld d=%d)", (long long)rows, d);
    if (rows == 0) return MME_OK;
    if (!shard || !all) return fail(c, MME_E_ARG, "mme_allgather: null pointer");
    if (const char* why = rccl_ready()) return fail(c, MME_E_COMM, "%s", why);
    HIP_TRY(c, hipSetDevice(c->device));
    Timed t(c, (hipStream_t)stream, KC_COMM);
    // bf16 rows travel as bytes (bit-exact whatever the RCCL build thinks of bf16 arithmetic)
    RCCL_TRY(c, rccl_allgather_bytes(shard, all, (size_t)rows * d * 2, comm, (hipStream_t)stream));
    return MME_OK;
}

int mme_attention_stamps(mme_ctx* c, int B, int iters, double* avg_ms, uint64_t* stamps_host) {
    if (!c || !avg_ms || !stamps_host || B <= 0 || iters < 1) return fail(c, MME_E_ARG, "mme_attention_stamps: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int heads = c->geom.heads;
    const size_t D = (size_t)c->geom.hidden, rows = (size_t)B * VIT_T, q_bytes = rows * 3 * D * 2, o_bytes = rows * D * 2, st_bytes = (size_t)B * 64 * sizeof(uint64_t);
    void *Q = nullptr, *O = nullptr, *ST = nullptr, *G = nullptr;
    int rc = MME_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    do {
        if (hipMalloc(&Q, q_bytes) != hipSuccess || hipMalloc(&O, o_bytes) != hipSuccess || hipMalloc(&ST, st_bytes) != hipSuccess || hipMalloc(&G, 256) != hipSuccess) { rc = fail(c, MME_E_NOMEM, "mme_attention_stamps: hipMalloc"); break; }
        (void)hipMemset(G, 0, 256);
        {   // uniform [-1, 1) bf16 activations, a 64 MB pattern repeated
            const size_t pat = (size_t)32 << 20;
            std::vector<uint16_t> h(pat);
            uint64_t x = 0x9E3779B97F4A7C15ull;
            for (size_t i = 0; i < pat; ++i) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                h[i] = f32_to_bf16_rne((float)((int64_t)(x >> 40) - (1 << 23)) * (1.0f / (1 << 23)));
            }
            for (size_t o = 0; o < q_bytes; o += pat * 2)
                if (hipMemcpy((char*)Q + o, h.data(), (q_bytes - o < pat * 2 ? q_bytes - o : pat * 2), hipMemcpyHostToDevice) != hipSuccess) { rc = fail(c, MME_E_HIP, "memcpy"); break; }
            if (rc) break;
        }
        hipStream_t s = nullptr;
        int* guard = c->attn_mode ? (int*)G : nullptr;  // mode 0: the exact kernel alone
        if (launch_attention(Q, O, B, heads, s, guard, c->attn_mode == 2) != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_attention_stamps: launch"); break; }
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; ++i) (void)launch_attention(Q, O, B, heads, s, guard, c->attn_mode == 2);
        (void)hipEventRecord(e1, s);
        if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_attention_stamps: kernel failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *avg_ms = ms / iters;
        (void)hipMemset(ST, 0, st_bytes);
        if (launch_attention_stamped(Q, O, B, heads, guard != nullptr, (unsigned long long*)ST, s) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { rc = fail(c, MME_E_HIP, "mme_attention_stamps: stamped launch"); break; }
        (void)hipMemcpy(stamps_host, ST, st_bytes, hipMemcpyDeviceToHost);
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (void* p : {Q, O, ST, G}) if (p) (void)hipFree(p);
    return rc;
}

int mme_profile_enable(mme_ctx* c, int on) {
    if (!c) return MME_E_ARG;
    c->prof = on != 0;
    return MME_OK;
}

int mme_profile_reset(mme_ctx* c) {
    if (!c) return MME_E_ARG;
    c->events_used = 0;
    return MME_OK;
}

int mme_profile_read_sync(mme_ctx* c, int count, double* ms, int64_t* launches) {
    if (!c || !ms || !launches || count < 0) return fail(c, MME_E_ARG, "mme_profile_read_sync: null argument or negative count");
    const int nc = count < MME_NUM_KERNEL_CLASSES ? count : MME_NUM_KERNEL_CLASSES;
    for (int i = 0; i < nc; ++i) {
        ms[i] = 0.0;
        launches[i] = 0;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    for (size_t i = 0; i < c->events_used; ++i) {
        EventPair& ev = c->events[i];
        HIP_TRY(c, hipEventSynchronize(ev.b));
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
        if (ev.cls >= nc) continue;  // a class the caller's arrays have no slot for
        ms[ev.cls] += t;
        launches[ev.cls] += 1;
    }
    return MME_NUM_KERNEL_CLASSES;
}

}  // extern "C"
