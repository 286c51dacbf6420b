// Weight loading: the two preparers (ctx.h) and the ViT/16 load sequence written once against them.
//   HostPrep   f32 host tensors, prepared by the loops below and uploaded buffer by buffer (mme_load_vit, mme_load_tile_vit)
//   DevPrep    the checkpoint's own bytes (f32, bf16 or f16) staged on the device, prepared by the kernels of
//              weight_prep.hip (mme_load_vit_as, mme_load_tile_vit_as)
// Every kernel keeps the operations of its host loop and their order: tests/test_gpu_checkpoint.py holds the two to equal
// fingerprints, tests/test_gpu_weight_prep.py compares what both prepared with float64 from the model's definition.  The tile-ViT sequence is prepare_tile in
// capi_tilevit.hip, beside the tower's device record.
#include <hip/hip_runtime.h>

#include <vector>

#include "ctx.h"

int check_load_dtype(mme_ctx* c, int dtype, const char* who) {
    if (dtype < MME_DT_F32 || dtype > MME_DT_F16) return fail(c, MME_E_ARG, "%s: dtype %d (MME_DT_F32 = 0, MME_DT_BF16 = 1, MME_DT_F16 = 2)", who, dtype);
    return MME_OK;
}

namespace {

// hipMalloc of n elements, registered in c->allocs / c->alloc_bytes: every prepared buffer of both preparers
template <class T>
int alloc_weight(mme_ctx* c, size_t n, T** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) return fail(c, MME_E_NOMEM, "hipMalloc weights: %s", hipGetErrorString(e));
    c->allocs.push_back(p);
    c->alloc_bytes.push_back(n * sizeof(T));
    *out = (T*)p;
    return MME_OK;
}

// ---- HostPrep ------------------------------------------------------------------------------------------------------------
template <class T>
int upload(mme_ctx* c, const void* h, size_t n, T** dst) {
    int r;
    if ((r = alloc_weight(c, n, dst))) return r;
    HIP_TRY(c, hipMemcpy(*dst, h, n * sizeof(T), hipMemcpyHostToDevice));
    return MME_OK;
}

// dst[i] = src[i] (* scale); the product is rounded to f32 here, before whatever follows
void copy_scaled(const float* src, size_t n, float scale, bool scaled, float* dst) {
    if (scaled)
        for (size_t i = 0; i < n; ++i) dst[i] = f32_quiet_nan(src[i] * scale);
    else
        for (size_t i = 0; i < n; ++i) dst[i] = f32_quiet_nan(src[i]);
}

}  // namespace

int HostPrep::table(const void* src, size_t n, float scale, bool scaled, float** dst) {
    return table_cat(&src, &n, 1, scale, scaled, dst);
}

int HostPrep::table_cat(const void* const* srcs, const size_t* n, int nsrc, float scale0, bool scaled0, float** dst) {
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += n[i];
    std::vector<float> h(total);
    size_t o = 0;
    for (int i = 0; i < nsrc; o += n[i], ++i) copy_scaled((const float*)srcs[i], n[i], scale0, scaled0 && i == 0, h.data() + o);
    return upload(c, h.data(), total, dst);
}

int HostPrep::bf16(const void* const* srcs, const size_t* rows, int nsrc, size_t cols, float scale0, bool scaled0, bf16_t** dst) {
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += rows[i] * cols;
    std::vector<uint16_t> h(total);
    size_t o = 0;
    for (int i = 0; i < nsrc; ++i) {
        const float* src = (const float*)srcs[i];
        const size_t n = rows[i] * cols;
        if (scaled0 && i == 0)
            for (size_t k = 0; k < n; ++k) h[o++] = f32_to_bf16_rne(src[k] * scale0);
        else
            for (size_t k = 0; k < n; ++k) h[o++] = f32_to_bf16_rne(src[k]);
    }
    return upload(c, h.data(), total, dst);
}

int HostPrep::folded(const WpFoldSrc* srcs, const size_t* rows, int nsrc, size_t cols, const void* gamma_, const void* beta_, bf16_t** wf, float** cs,
                     float** bf) {
    const float *gamma = (const float*)gamma_, *beta = (const float*)beta_;
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += rows[i];
    std::vector<uint16_t> hw(total * cols);
    std::vector<float> hcs(total), hbf(total);
    size_t o = 0;
    for (int i = 0; i < nsrc; ++i) {
        const float *ws = (const float*)srcs[i].w, *bs = (const float*)srcs[i].b;
        const float scale = srcs[i].scale;
        const bool scaled = srcs[i].scaled != 0;
        for (size_t n = 0; n < rows[i]; ++n, ++o) {
            double s = 0.0, t = 0.0;
            for (size_t k = 0; k < cols; ++k) {
                const float w = scaled ? ws[n * cols + k] * scale : ws[n * cols + k];
                const uint16_t q = f32_to_bf16_rne(w * gamma[k]);
                hw[o * cols + k] = q;
                uint32_t u = (uint32_t)q << 16;
                float wq;
                memcpy(&wq, &u, 4);
                s += (double)wq;
                t += (double)w * (double)beta[k];
            }
            const float b = !bs ? 0.f : (scaled ? bs[n] * scale : bs[n]);
            hcs[o] = (float)s;
            hbf[o] = (float)((double)b + t);
        }
    }
    int r;
    if ((r = upload(c, hw.data(), hw.size(), wf))) return r;
    if ((r = upload(c, hcs.data(), total, cs))) return r;
    return upload(c, hbf.data(), total, bf);
}

int HostPrep::padded(const void* src, int rows, int cols, int cols_padded, bf16_t** dst) {
    std::vector<uint16_t> h((size_t)rows * cols_padded, 0);  // bf16 +0.0
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < cols; ++k) h[(size_t)n * cols_padded + k] = f32_to_bf16_rne(((const float*)src)[(size_t)n * cols + k]);
    return upload(c, h.data(), h.size(), dst);
}

int HostPrep::rowscaled(const void* src, size_t rows, size_t cols, const void* factor, bf16_t** dst) {
    std::vector<uint16_t> h(rows * cols);
    for (size_t n = 0; n < rows; ++n) {
        const float f = ((const float*)factor)[n];
        for (size_t k = 0; k < cols; ++k) h[n * cols + k] = f32_to_bf16_rne(f * ((const float*)src)[n * cols + k]);
    }
    return upload(c, h.data(), h.size(), dst);
}

int HostPrep::table_mul(const void* src, const void* factor, size_t n, float** dst) {
    std::vector<float> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = f32_quiet_nan(((const float*)factor)[i] * ((const float*)src)[i]);
    return upload(c, h.data(), n, dst);
}

int HostPrep::zeros(size_t n, float** dst) {
    std::vector<float> z(n, 0.f);
    return upload(c, z.data(), n, dst);
}

// ---- DevPrep -------------------------------------------------------------------------------------------------------------
int WeightStage::reserve(mme_ctx* c) {
    hipError_t e = hipMalloc((void**)&base, used ? used : 16);
    if (e != hipSuccess) return fail(c, MME_E_NOMEM, "hipMalloc(%zu) for the staged checkpoint bytes: %s", used, hipGetErrorString(e));
    total = used;
    used = 0;
    dry = false;
    return MME_OK;
}

const void* WeightStage::put(const void* host, size_t n) {
    const size_t bytes = n * esz, off = used;
    used += (bytes + 15) & ~(size_t)15;
    if (dry) return host;
    if (err != hipSuccess) return nullptr;
    if (used > total) {
        err = hipErrorInvalidValue;
        return nullptr;
    }
    err = hipMemcpyAsync(base + off, host, bytes, hipMemcpyHostToDevice, s);
    return base + off;
}

void WeightStage::release() {
    if (base) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(base);
    }
    base = nullptr;
}

int DevPrep::finish(int r) {
    if (r == MME_OK) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) r = fail(c, MME_E_HIP, "%s: weight preparation: %s", who, hipGetErrorString(e));
    }
    st.release();
    return r;
}

int DevPrep::table(const void* src, size_t n, float scale, bool scaled, float** dst) { return table_cat(&src, &n, 1, scale, scaled, dst); }

int DevPrep::table_cat(const void* const* srcs, const size_t* n, int nsrc, float scale0, bool scaled0, float** dst) {
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += n[i];
    int r;
    if ((r = alloc_weight(c, total, dst))) return r;
    size_t o = 0;
    for (int i = 0; i < nsrc; o += n[i], ++i)  // one launch per part into its slice
        HIP_TRY(c, launch_wp_convert(dt, srcs[i], n[i], scale0, scaled0 && i == 0, false, *dst + o, s));
    return MME_OK;
}

int DevPrep::bf16(const void* const* srcs, const size_t* rows, int nsrc, size_t cols, float scale0, bool scaled0, bf16_t** dst) {
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += rows[i] * cols;
    int r;
    if ((r = alloc_weight(c, total, dst))) return r;
    size_t o = 0;
    for (int i = 0; i < nsrc; o += rows[i] * cols, ++i)
        HIP_TRY(c, launch_wp_convert(dt, srcs[i], rows[i] * cols, scale0, scaled0 && i == 0, true, *dst + o, s));
    return MME_OK;
}

int DevPrep::folded(const WpFoldSrc* srcs, const size_t* rows, int nsrc, size_t cols, const void* gamma, const void* beta, bf16_t** wf, float** cs,
                    float** bf) {
    size_t total = 0;
    for (int i = 0; i < nsrc; ++i) total += rows[i];
    int r;
    if ((r = alloc_weight(c, total * cols, wf))) return r;
    if ((r = alloc_weight(c, total, cs))) return r;
    if ((r = alloc_weight(c, total, bf))) return r;
    HIP_TRY(c, launch_wp_fold(dt, srcs, rows, nsrc, (int)cols, gamma, beta, *wf, *cs, *bf, s));
    return MME_OK;
}

int DevPrep::padded(const void* src, int rows, int cols, int cols_padded, bf16_t** dst) {
    int r;
    if ((r = alloc_weight(c, (size_t)rows * cols_padded, dst))) return r;
    HIP_TRY(c, launch_wp_pad(dt, src, rows, cols, cols_padded, *dst, s));
    return MME_OK;
}

int DevPrep::rowscaled(const void* src, size_t rows, size_t cols, const void* factor, bf16_t** dst) {
    int r;
    if ((r = alloc_weight(c, rows * cols, dst))) return r;
    HIP_TRY(c, launch_wp_rowscale(dt, src, rows, cols, factor, *dst, s));
    return MME_OK;
}

int DevPrep::table_mul(const void* src, const void* factor, size_t n, float** dst) {
    int r;
    if ((r = alloc_weight(c, n, dst))) return r;
    HIP_TRY(c, launch_wp_mul(dt, src, factor, n, *dst, s));
    return MME_OK;
}

int DevPrep::zeros(size_t n, float** dst) {
    int r;
    if ((r = alloc_weight(c, n, dst))) return r;
    HIP_TRY(c, hipMemsetAsync(*dst, 0, n * sizeof(float), s));
    return MME_OK;
}

// ---- ViT/16, ViT/32 --------------------------------------------------------------------------------------------------------------
namespace {

// argument checks of both ViT loaders (the messages of both name the f32 loader): the geometry against the supported
// set, every tensor pointer.  Touches nothing in the context but its error text.
// no_cls: a tower without a class token (SigLIP): patch 16 only, cls_token NULL
// p14: the DINOv2 loader, patch 14 only; every other loader keeps refusing patch 14
int validate_vit_weights(mme_ctx* c, const mme_vit_weights* w, const char* who = "mme_load_vit", bool bias_free_patch = false, bool no_cls = false,
                         bool p14 = false) {
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    // every refusal names the field, the value found and what is supported
    if (w->image_size != VIT_IMG) return fail(c, MME_E_ARG, "%s: image_size = %d; supported: %d", who, w->image_size, VIT_IMG);
    if (no_cls && w->patch_size != 16) return fail(c, MME_E_ARG, "%s: patch_size = %d; supported: 16", who, w->patch_size);
    if (p14 && w->patch_size != 14) return fail(c, MME_E_ARG, "%s: patch_size = %d; supported: 14", who, w->patch_size);
    if (!p14 && w->patch_size != 16 && w->patch_size != 32) return fail(c, MME_E_ARG, "%s: patch_size = %d; supported: 16, 32", who, w->patch_size);
    if (!vit_width_built(w->hidden)) return fail(c, MME_E_ARG, "%s: hidden = %d; supported: 384, 768, 1024", who, w->hidden);
    if (w->heads * VIT_DH != w->hidden)
        return fail(c, MME_E_ARG, "%s: heads = %d at hidden = %d; supported: heads of %d, heads = hidden / %d = %d", who, w->heads, w->hidden, VIT_DH, VIT_DH,
                    w->hidden / VIT_DH);
    if (w->mlp < 64 || (w->mlp % 64) != 0 || w->mlp > VIT_MAX_F)
        return fail(c, MME_E_ARG, "%s: mlp = %d; supported: multiples of 64 up to %d", who, w->mlp, VIT_MAX_F);
    if (w->layers < 1 || w->layers > VIT_MAX_L) return fail(c, MME_E_ARG, "%s: layers = %d; supported: 1..%d", who, w->layers, VIT_MAX_L);
    if (no_cls && w->cls_token) return fail(c, MME_E_ARG, "%s: vit.cls_token is set; supported: NULL (the tower has no class token)", who);
    if ((!w->cls_token && !no_cls) || !w->pos_emb || !w->patch_w || (!w->patch_b && !bias_free_patch) || !w->lnf_g || !w->lnf_b || !w->layer)
        return fail(c, MME_E_ARG, "%s: null tensor pointer", who);
    for (int l = 0; l < w->layers; ++l) {
        const mme_vit_layer& a = w->layer[l];
        const float* all[] = {a.ln1_g, a.ln1_b, a.q_w, a.q_b, a.k_w, a.k_b, a.v_w, a.v_b, a.o_w, a.o_b, a.ln2_g, a.ln2_b, a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b};
        for (const float* p : all)
            if (!p) return fail(c, MME_E_ARG, "%s: layer %d has a null tensor pointer", who, l);
    }
    return MME_OK;
}

// A load replaces what the context held: begin frees the previous ViT weights (after the device has drained), takes the
// new geometry and leaves the context unloaded; end marks the buffers allocated since as the ViT weights and, when
// `ok`, the context as loaded.  A load that fails in between leaves the context without weights.
int begin_vit_load(mme_ctx* c, const mme_vit_weights* w) {
    HIP_TRY(c, hipSetDevice(c->device));
    c->loaded = false;
    c->pool_mode = MME_POOL_TOKEN;  // mme_set_pooling holds until the next load
    if (c->vit_alloc_hi > c->vit_alloc_lo) HIP_TRY(c, hipDeviceSynchronize());  // a pass in flight still reads them
    // exactly the image tower's buffers; a text tower loaded behind them keeps its own, its range moves down with them
    release_alloc_range(c, c->vit_alloc_lo, c->vit_alloc_hi);
    c->geom = VitGeom{w->hidden, w->layers, w->heads, w->mlp, w->patch_size, w->cls_token == nullptr};  // no class token: SigLIP only (validated)
    c->ln_eps = w->ln_eps;
    c->layer.assign((size_t)w->layers, LayerDev{});
    // a plain ViT until a CLIP load says otherwise (load_clip sets these after this call; their buffers were freed above)
    c->clip = false;
    c->act = 0;
    c->proj_dim = 0;
    c->pre_g = c->pre_b = nullptr;
    c->proj_w = nullptr;
    c->siglip = false;
    c->dinov2 = false;
    c->head = LayerDev{};
    c->head_q = nullptr;
    return MME_OK;
}

void end_vit_load(mme_ctx* c, bool ok) {
    c->vit_alloc_hi = c->allocs.size();
    c->loaded = ok;
}

// every tensor of the checkpoint with its element count (the order of the staged bytes)
// pos_on_host: the position table is not staged (DINOv2: the loader's interpolated f32 table, whatever the checkpoint's type)
template <class Fn>
void each_vit_tensor(mme_vit_weights& w, std::vector<mme_vit_layer>& layer, Fn&& f, bool pos_on_host = false) {
    const size_t D = (size_t)w.hidden, F = (size_t)w.mlp;
    const VitGeom vg{w.hidden, w.layers, w.heads, w.mlp, w.patch_size, w.cls_token == nullptr};
    if (w.cls_token) f(w.cls_token, D);  // SigLIP: no class token
    if (!pos_on_host) f(w.pos_emb, (size_t)vg.tokens() * D);
    f(w.patch_w, D * vg.patch_elems());
    if (w.patch_b) f(w.patch_b, D);  // CLIP: no bias on the patch projection
    f(w.lnf_g, D);
    f(w.lnf_b, D);
    for (mme_vit_layer& a : layer) {
        f(a.ln1_g, D); f(a.ln1_b, D);
        f(a.q_w, D * D); f(a.q_b, D);
        f(a.k_w, D * D); f(a.k_b, D);
        f(a.v_w, D * D); f(a.v_b, D);
        f(a.o_w, D * D); f(a.o_b, D);
        f(a.ln2_g, D); f(a.ln2_b, D);
        f(a.fc1_w, F * D); f(a.fc1_b, F);
        f(a.fc2_w, D * F); f(a.fc2_b, D);
    }
}

// The prepared buffers of the ViT/16 encoder, in the order mme_weights_fingerprint reports them: cls, pos, patch_b, lnf_g,
// lnf_b, patch_w, then 18 per layer.
// ls (DINOv2 only, [layers]): LayerScale folded into the projection it follows, o_w' = bf16(lambda1 * o_w), o_b' = lambda1 * o_b and
// the same for fc2 with lambda2 (the block then runs unchanged); the position table is the caller's host f32 under both
// preparers, and patch_w [D, 588] is padded to [D, 640].  The order and the count of the buffers are the ViT's.
template <class P>
int prepare_vit(mme_ctx* c, P& p, const mme_vit_weights& w, const mme_dinov2_scale* ls = nullptr) {
    int r;
    const size_t D = (size_t)w.hidden, F = (size_t)w.mlp;
    const size_t rD[3] = {D, D, D}, rF[1] = {F};
    const VitGeom vg{w.hidden, w.layers, w.heads, w.mlp, w.patch_size, w.cls_token == nullptr};  // pos [197 | 50 | 196, D], patch_w [D, 768 | 3072]
    auto plain = [&](const float* src, size_t n, float** dst) { return p.table(src, n, 1.f, false, dst); };
    auto plain_bf16 = [&](const float* src, const size_t* rows, size_t cols, bf16_t** dst) {
        const void* s[1] = {src};
        return p.bf16(s, rows, 1, cols, 1.f, false, dst);
    };
    if ((r = w.cls_token ? plain(w.cls_token, D, &c->cls) : p.zeros(D, &c->cls))) return r;  // SigLIP: a zero table, never read
    if (ls) {
        HostPrep hp{c};
        if ((r = hp.table(w.pos_emb, (size_t)vg.tokens() * D, 1.f, false, &c->pos))) return r;
    } else if ((r = plain(w.pos_emb, (size_t)vg.tokens() * D, &c->pos))) return r;
    if ((r = w.patch_b ? plain(w.patch_b, D, &c->patch_b) : p.zeros(D, &c->patch_b))) return r;  // CLIP: a zero table
    if ((r = plain(w.lnf_g, D, &c->lnf_g))) return r;
    if ((r = plain(w.lnf_b, D, &c->lnf_b))) return r;
    if (vg.patch_elems() != vg.patch_dim()) {  // patch 14: 588 -> 640
        if ((r = p.padded(w.patch_w, (int)D, vg.patch_elems(), vg.patch_dim(), &c->patch_w))) return r;
    } else if ((r = plain_bf16(w.patch_w, rD, (size_t)vg.patch_dim(), &c->patch_w))) return r;
    // The attention kernel takes its scores in log2 units straight from the matrix pipe (attention.hip, PRESCALED):
    // dh^-0.5 * log2(e) is folded into the query projection here, once, BEFORE the rounding to bf16 that the preparation
    // applies anyway -- softmax(q.k / 8) = exp2(q'.k - c) / sum with q' = (W_q' x + b_q'), W_q' = sc W_q, b_q' = sc b_q.
    const float sc = 0.125f * 1.44269504088896341f;
    for (int l = 0; l < w.layers; ++l) {
        const mme_vit_layer& a = w.layer[l];
        LayerDev& L = c->layer[l];
        if ((r = plain(a.ln1_g, D, &L.ln1_g))) return r;
        if ((r = plain(a.ln1_b, D, &L.ln1_b))) return r;
        if ((r = plain(a.ln2_g, D, &L.ln2_g))) return r;
        if ((r = plain(a.ln2_b, D, &L.ln2_b))) return r;
        const void* qkv[3] = {a.q_w, a.k_w, a.v_w};
        if ((r = p.bf16(qkv, rD, 3, D, sc, true, &L.qkv_w))) return r;
        const void* qkvb[3] = {a.q_b, a.k_b, a.v_b};
        if ((r = p.table_cat(qkvb, rD, 3, sc, true, &L.qkv_b))) return r;
        const WpFoldSrc fq[3] = {{a.q_w, a.q_b, sc, 1}, {a.k_w, a.k_b, 1.f, 0}, {a.v_w, a.v_b, 1.f, 0}};
        if ((r = p.folded(fq, rD, 3, D, a.ln1_g, a.ln1_b, &L.w.qkv_wf, &L.w.qkv_cs, &L.w.qkv_bf))) return r;
        if ((r = ls ? p.rowscaled(a.o_w, D, D, ls[l].lambda1, &L.w.o_w) : plain_bf16(a.o_w, rD, D, &L.w.o_w))) return r;
        if ((r = ls ? p.table_mul(a.o_b, ls[l].lambda1, D, &L.w.o_b) : plain(a.o_b, D, &L.w.o_b))) return r;
        if ((r = plain_bf16(a.fc1_w, rF, D, &L.fc1_w))) return r;
        if ((r = plain(a.fc1_b, F, &L.fc1_b))) return r;
        const WpFoldSrc f1[1] = {{a.fc1_w, a.fc1_b, 1.f, 0}};
        if ((r = p.folded(f1, rF, 1, D, a.ln2_g, a.ln2_b, &L.w.fc1_wf, &L.w.fc1_cs, &L.w.fc1_bf))) return r;
        if ((r = ls ? p.rowscaled(a.fc2_w, D, F, ls[l].lambda2, &L.w.fc2_w) : plain_bf16(a.fc2_w, rD, F, &L.w.fc2_w))) return r;
        if ((r = ls ? p.table_mul(a.fc2_b, ls[l].lambda2, D, &L.w.fc2_b) : plain(a.fc2_b, D, &L.w.fc2_b))) return r;
    }
    return MME_OK;
}

template <class P>
int load_vit(mme_ctx* c, const mme_vit_weights* w, P p) {
    int r;
    if ((r = begin_vit_load(c, w))) return r;
    // the preparer's view of the tensors: the caller's pointers, or where the preparer staged them
    std::vector<mme_vit_layer> layer(w->layer, w->layer + w->layers);
    mme_vit_weights v = *w;
    v.layer = layer.data();
    r = p.stage([&](auto& put) { each_vit_tensor(v, layer, put); });
    if (r == MME_OK) r = prepare_vit(c, p, v);
    r = p.finish(r);
    end_vit_load(c, r == MME_OK);
    return r;
}

// ---- CLIP image tower: the ViT sequence, then pre_g, pre_b [D] and proj_w bf16 [P, D] -------------------------------------------
int validate_clip_weights(mme_ctx* c, const mme_clip_weights* w) {
    const char* who = "mme_load_clip";
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    int r;
    if ((r = validate_vit_weights(c, &w->vit, who, true))) return r;
    if (!w->pre_g || !w->pre_b) return fail(c, MME_E_ARG, "%s: pre_g / pre_b (pre_layrnorm) is a null tensor pointer", who);
    if (w->act != 0 && w->act != 1) return fail(c, MME_E_ARG, "%s: act = %d; supported: 0 (erf-GELU), 1 (QuickGELU)", who, w->act);
    if (w->proj_dim != 0 && (w->proj_dim < 64 || (w->proj_dim % 64) != 0 || w->proj_dim > 1024))
        return fail(c, MME_E_ARG, "%s: proj_dim = %d; supported: 0 (no projection) or a multiple of 64 up to 1024", who, w->proj_dim);
    if ((w->proj_dim != 0) != (w->proj_w != nullptr))
        return fail(c, MME_E_ARG, "%s: proj_dim = %d with proj_w %s; supported: both set, or proj_dim = 0 with proj_w NULL", who, w->proj_dim,
                    w->proj_w ? "set" : "NULL");
    return MME_OK;
}

template <class P>
int prepare_clip(mme_ctx* c, P& p, const mme_clip_weights& w) {
    int r;
    const size_t D = (size_t)w.vit.hidden;
    if ((r = prepare_vit(c, p, w.vit))) return r;
    if ((r = p.table(w.pre_g, D, 1.f, false, &c->pre_g))) return r;
    if ((r = p.table(w.pre_b, D, 1.f, false, &c->pre_b))) return r;
    if (w.proj_w) {
        const void* s[1] = {w.proj_w};
        const size_t rows[1] = {(size_t)w.proj_dim};
        if ((r = p.bf16(s, rows, 1, D, 1.f, false, &c->proj_w))) return r;
    }
    return MME_OK;
}

template <class P>
int load_clip(mme_ctx* c, const mme_clip_weights* w, P p) {
    int r;
    if ((r = begin_vit_load(c, &w->vit))) return r;
    std::vector<mme_vit_layer> layer(w->vit.layer, w->vit.layer + w->vit.layers);
    mme_clip_weights v = *w;
    v.vit.layer = layer.data();
    r = p.stage([&](auto& put) {
        each_vit_tensor(v.vit, layer, put);
        put(v.pre_g, (size_t)v.vit.hidden);
        put(v.pre_b, (size_t)v.vit.hidden);
        if (v.proj_w) put(v.proj_w, (size_t)v.proj_dim * v.vit.hidden);
    });
    if (r == MME_OK) r = prepare_clip(c, p, v);
    r = p.finish(r);
    if (r == MME_OK) {
        c->clip = true;
        c->act = w->act;
        c->proj_dim = w->proj_dim;
    }
    end_vit_load(c, r == MME_OK);
    return r;
}

// ---- SigLIP image tower: the ViT sequence (no class token), then the pooling head -----------------------------------------------
int validate_siglip_weights(mme_ctx* c, const mme_siglip_weights* w) {
    const char* who = "mme_load_siglip";
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    int r;
    if ((r = validate_vit_weights(c, &w->vit, who, false, true))) return r;
    if (!w->probe) return fail(c, MME_E_ARG, "%s: probe is a null tensor pointer", who);
    const mme_vit_layer& a = w->head;  // ln1_g / ln1_b are not read
    const float* all[] = {a.q_w, a.q_b, a.k_w, a.k_b, a.v_w, a.v_b, a.o_w, a.o_b, a.ln2_g, a.ln2_b, a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b};
    for (const float* p : all)
        if (!p) return fail(c, MME_E_ARG, "%s: head has a null tensor pointer", who);
    return MME_OK;
}

// The head's tensors with their element counts, behind the ViT's in the staged bytes
template <class Fn>
void each_siglip_head_tensor(mme_siglip_weights& w, Fn&& f) {
    const size_t D = (size_t)w.vit.hidden, F = (size_t)w.vit.mlp;
    mme_vit_layer& a = w.head;
    f(w.probe, D);
    f(a.q_w, D * D); f(a.q_b, D);
    f(a.k_w, D * D); f(a.k_b, D);
    f(a.v_w, D * D); f(a.v_b, D);
    f(a.o_w, D * D); f(a.o_b, D);
    f(a.ln2_g, D); f(a.ln2_b, D);
    f(a.fc1_w, F * D); f(a.fc1_b, F);
    f(a.fc2_w, D * F); f(a.fc2_b, D);
}

// Prepared buffers behind the ViT's 6 + 18 L: the head's ln2_g, ln2_b, K | V bf16 [2 D, D], their bias [2 D], the K | V fold
// with post_layernorm (wf, cs, bf), the query's three (below), o_w, o_b, fc1_w, fc1_b, the fc1 fold (wf, cs, bf), fc2_w, fc2_b.
template <class P>
int prepare_siglip(mme_ctx* c, P& p, const mme_siglip_weights& w) {
    int r;
    const size_t D = (size_t)w.vit.hidden, F = (size_t)w.vit.mlp;
    const size_t rD[2] = {D, D}, rF[1] = {F};
    if ((r = prepare_vit(c, p, w.vit))) return r;
    auto plain = [&](const float* src, size_t n, float** dst) { return p.table(src, n, 1.f, false, dst); };
    auto plain_bf16 = [&](const float* src, const size_t* rows, size_t cols, bf16_t** dst) {
        const void* s[1] = {src};
        return p.bf16(s, rows, 1, cols, 1.f, false, dst);
    };
    const mme_vit_layer& a = w.head;
    LayerDev& L = c->head;
    if ((r = plain(a.ln2_g, D, &L.ln2_g))) return r;
    if ((r = plain(a.ln2_b, D, &L.ln2_b))) return r;
    const void* kv[2] = {a.k_w, a.v_w};
    if ((r = p.bf16(kv, rD, 2, D, 1.f, false, &L.qkv_w))) return r;
    const void* kvb[2] = {a.k_b, a.v_b};
    if ((r = p.table_cat(kvb, rD, 2, 1.f, false, &L.qkv_b))) return r;
    // K | V of the head read post_layernorm(x): that LayerNorm is folded into them as ln1 is into a block's QKV
    const WpFoldSrc fkv[2] = {{a.k_w, a.k_b, 1.f, 0}, {a.v_w, a.v_b, 1.f, 0}};
    if ((r = p.folded(fkv, rD, 2, D, w.vit.lnf_g, w.vit.lnf_b, &L.w.qkv_wf, &L.w.qkv_cs, &L.w.qkv_bf))) return r;
    // The query is the same for every crop: q = sc (probe . W_q^T + b_q), sc = dh^-0.5 log2 e applied to W_q and b_q in f32
    // first, as a block's query rows are.  That is the bias' of the fold, b' = b + sum_k w beta_k (f64, k ascending), with
    // the probe standing in for beta, so both preparers compute it with the operation they share; the fold's other two
    // outputs (W_q times post_layernorm's gamma, its column sums) are prepared and not read.
    const float sc = 0.125f * 1.44269504088896341f;
    const WpFoldSrc fq[1] = {{a.q_w, a.q_b, sc, 1}};
    bf16_t* q_wf_unused;
    float* q_cs_unused;
    if ((r = p.folded(fq, rD, 1, D, w.vit.lnf_g, w.probe, &q_wf_unused, &q_cs_unused, &c->head_q))) return r;
    if ((r = plain_bf16(a.o_w, rD, D, &L.w.o_w))) return r;
    if ((r = plain(a.o_b, D, &L.w.o_b))) return r;
    if ((r = plain_bf16(a.fc1_w, rF, D, &L.fc1_w))) return r;
    if ((r = plain(a.fc1_b, F, &L.fc1_b))) return r;
    const WpFoldSrc f1[1] = {{a.fc1_w, a.fc1_b, 1.f, 0}};
    if ((r = p.folded(f1, rF, 1, D, a.ln2_g, a.ln2_b, &L.w.fc1_wf, &L.w.fc1_cs, &L.w.fc1_bf))) return r;
    if ((r = plain_bf16(a.fc2_w, rD, F, &L.w.fc2_w))) return r;
    return plain(a.fc2_b, D, &L.w.fc2_b);
}

template <class P>
int load_siglip(mme_ctx* c, const mme_siglip_weights* w, P p) {
    int r;
    if ((r = begin_vit_load(c, &w->vit))) return r;
    std::vector<mme_vit_layer> layer(w->vit.layer, w->vit.layer + w->vit.layers);
    mme_siglip_weights v = *w;
    v.vit.layer = layer.data();
    r = p.stage([&](auto& put) {
        each_vit_tensor(v.vit, layer, put);
        each_siglip_head_tensor(v, put);
    });
    if (r == MME_OK) r = prepare_siglip(c, p, v);
    r = p.finish(r);
    if (r == MME_OK) {
        c->siglip = true;
        c->act = 2;
    }
    end_vit_load(c, r == MME_OK);
    return r;
}

// ---- DINOv2 image tower: the ViT sequence at patch 14 with LayerScale folded in ---------------------------------------------------
int validate_dinov2_weights(mme_ctx* c, const mme_dinov2_weights* w) {
    const char* who = "mme_load_dinov2";
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    int r;
    if ((r = validate_vit_weights(c, &w->vit, who, false, false, true))) return r;
    if (!w->scale) return fail(c, MME_E_ARG, "%s: scale is a null pointer", who);
    for (int l = 0; l < w->vit.layers; ++l)
        if (!w->scale[l].lambda1 || !w->scale[l].lambda2) return fail(c, MME_E_ARG, "%s: layer %d has a null LayerScale pointer", who, l);
    return MME_OK;
}

template <class P>
int load_dinov2(mme_ctx* c, const mme_dinov2_weights* w, P p) {
    int r;
    if ((r = begin_vit_load(c, &w->vit))) return r;
    std::vector<mme_vit_layer> layer(w->vit.layer, w->vit.layer + w->vit.layers);
    std::vector<mme_dinov2_scale> scale(w->scale, w->scale + w->vit.layers);
    mme_vit_weights v = w->vit;
    v.layer = layer.data();
    r = p.stage([&](auto& put) {
        each_vit_tensor(v, layer, put, true);
        for (mme_dinov2_scale& sc : scale) {
            put(sc.lambda1, (size_t)v.hidden);
            put(sc.lambda2, (size_t)v.hidden);
        }
    });
    if (r == MME_OK) r = prepare_vit(c, p, v, scale.data());
    r = p.finish(r);
    if (r == MME_OK) c->dinov2 = true;
    end_vit_load(c, r == MME_OK);
    return r;
}

}  // namespace

extern "C" {

int mme_load_dinov2(mme_ctx* c, const mme_dinov2_weights* w) {
    int r;
    if ((r = validate_dinov2_weights(c, w))) return r;
    return load_dinov2(c, w, HostPrep{c});
}

int mme_load_dinov2_as(mme_ctx* c, const mme_dinov2_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_dinov2_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_dinov2_as"))) return r;
    return load_dinov2(c, w, DevPrep(c, dtype, stream, "mme_load_dinov2_as"));
}

int mme_load_siglip(mme_ctx* c, const mme_siglip_weights* w) {
    int r;
    if ((r = validate_siglip_weights(c, w))) return r;
    return load_siglip(c, w, HostPrep{c});
}

int mme_load_siglip_as(mme_ctx* c, const mme_siglip_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_siglip_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_siglip_as"))) return r;
    return load_siglip(c, w, DevPrep(c, dtype, stream, "mme_load_siglip_as"));
}

int mme_load_clip(mme_ctx* c, const mme_clip_weights* w) {
    int r;
    if ((r = validate_clip_weights(c, w))) return r;
    return load_clip(c, w, HostPrep{c});
}

int mme_load_clip_as(mme_ctx* c, const mme_clip_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_clip_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_clip_as"))) return r;
    return load_clip(c, w, DevPrep(c, dtype, stream, "mme_load_clip_as"));
}

int mme_load_vit(mme_ctx* c, const mme_vit_weights* w) {
    int r;
    if ((r = validate_vit_weights(c, w))) return r;
    return load_vit(c, w, HostPrep{c});
}

int mme_load_vit_as(mme_ctx* c, const mme_vit_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_vit_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_vit_as"))) return r;
    return load_vit(c, w, DevPrep(c, dtype, stream, "mme_load_vit_as"));
}

}  // extern "C"
