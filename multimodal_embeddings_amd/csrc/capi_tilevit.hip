// C ABI of the tile-ViT encoder option: the reference encoder's own vision tower geometry
// (deprecated_package/config.py:58 -> transformers MllamaVisionModel: <= 4 tiles of 560 x 560, patch 14, 1601 tokens per
// tile, 1280-d, 16 heads, 32 local + 8 gated global layers, 7680-d output) on the same MFMA GEMM, LayerNorm-folding
// and statistics machinery as the ViT-B/16 path, with its own flash-style attention kernel (attention_tiles.hip).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "encoder_pass.h"

namespace {
constexpr int TD = 1280, TF = 5120, TH = 16, TTOK = 1601, TTOKP = 1608, TTILES = 4, TT = TTILES * TTOKP, TGRID = 40;
constexpr int TPDIM = 588, TPDIMP = 640, TMAXI = 8, TARATIOS = 9;
}  // namespace

struct TileVitDev {
    int layers = 0, global_layers = 0, ni = 0;
    int inter_after[TMAXI];
    int save_before = 0;  // mme_tile_vit_weights.intermediate_save_point
    float eps = 1e-5f;
    float *cls = nullptr, *pre = nullptr, *pos = nullptr, *tilepos = nullptr, *post = nullptr;
    float *lnpre_g = nullptr, *lnpre_b = nullptr, *lnpost_g = nullptr, *lnpost_b = nullptr, *zeros = nullptr;
    bf16_t* patch_w = nullptr;
    std::vector<BlockW> layer;  // the prepared buffers are registered in the context (c->allocs)
    // workspace for `ws_images` images
    int ws_images = 0;
    DevBuf patches, pemb, x, qkv, att, mlp, stats, lnpart, inter, meta;
};

void tile_vit_free(mme_ctx* c) {
    if (!c->tv) return;
    TileVitDev* t = c->tv;
    DevBuf* bufs[] = {&t->patches, &t->pemb, &t->x, &t->qkv, &t->att, &t->mlp, &t->stats, &t->lnpart, &t->inter, &t->meta};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    delete t;
    c->tv = nullptr;
}

int tile_vit_states(mme_ctx* c, const char* who, const void** x, const void** inter, int* ni, int64_t* inter_stride) {
    if (!c->tv) return fail(c, MME_E_STATE, "%s: call mme_load_tile_vit first", who);
    const TileVitDev* t = c->tv;
    *x = t->x.p;
    *inter = t->ni ? t->inter.p : nullptr;
    *ni = t->ni;
    *inter_stride = (int64_t)t->ws_images * TT * TD;
    return MME_OK;
}

namespace {

int validate_tile_weights(mme_ctx* c, const mme_tile_vit_weights* w) {
    if (!c || !w) return fail(c, MME_E_ARG, "mme_load_tile_vit: null argument");
    if (w->image_size != 560 || w->patch_size != 14 || w->hidden != TD || w->heads != TH || w->mlp != TF || w->max_tiles != TTILES ||
        w->aspect_ratios != TARATIOS)
        return fail(c, MME_E_ARG, "mme_load_tile_vit: only the Mllama vision geometry 560/14/1280/16/5120, 4 tiles, 9 aspect-ratio rows is built; got %d/%d/%d/%d/%d, %d tiles, %d rows",
                    w->image_size, w->patch_size, w->hidden, w->heads, w->mlp, w->max_tiles, w->aspect_ratios);
    if (w->layers < 1 || w->global_layers < 0 || w->layers + w->global_layers > 256 || w->n_intermediate < 0 || w->n_intermediate > TMAXI)
        return fail(c, MME_E_ARG, "mme_load_tile_vit: bad layer counts (%d local, %d global, %d intermediate)", w->layers, w->global_layers, w->n_intermediate);
    for (int k = 0; k < w->n_intermediate; ++k)
        if (w->intermediate[k] < 0 || w->intermediate[k] >= w->layers || (k && w->intermediate[k] <= w->intermediate[k - 1]))
            return fail(c, MME_E_ARG, "mme_load_tile_vit: intermediate layer indices must be ascending and inside the local stack");
    if (w->intermediate_save_point != MME_TILE_SAVE_AFTER_LAYER && w->intermediate_save_point != MME_TILE_SAVE_BEFORE_LAYER)
        return fail(c, MME_E_ARG, "mme_load_tile_vit: intermediate_save_point must be MME_TILE_SAVE_AFTER_LAYER (0) or MME_TILE_SAVE_BEFORE_LAYER (1), got %d",
                    w->intermediate_save_point);
    if (!w->class_embedding || !w->patch_w || !w->pos_emb || !w->tile_pos_emb || !w->pre_emb || !w->post_emb || !w->ln_pre_g || !w->ln_pre_b ||
        !w->ln_post_g || !w->ln_post_b || !w->layer)
        return fail(c, MME_E_ARG, "mme_load_tile_vit: null tensor pointer");
    if (c->tv) return fail(c, MME_E_STATE, "mme_load_tile_vit: tile-ViT weights already loaded; create a new context");
    for (int l = 0; l < w->layers + w->global_layers; ++l) {
        const mme_tile_layer& a = w->layer[l];
        const float* all[] = {a.ln1_g, a.ln1_b, a.q_w, a.k_w, a.v_w, a.o_w, a.ln2_g, a.ln2_b, a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b};
        for (const float* p : all)
            if (!p) return fail(c, MME_E_ARG, "mme_load_tile_vit: layer %d has a null tensor pointer", l);
    }
    return MME_OK;
}

// the context's tower record with the layer counts of `w` (the prepared buffers follow)
int new_tile_dev(mme_ctx* c, const mme_tile_vit_weights* w) {
    HIP_TRY(c, hipSetDevice(c->device));
    TileVitDev* t = new (std::nothrow) TileVitDev();
    if (!t) return fail(c, MME_E_NOMEM, "mme_load_tile_vit: out of host memory");
    c->tv = t;
    c->pool_mode = MME_POOL_TOKEN;  // as every image-tower load
    t->layers = w->layers;
    t->global_layers = w->global_layers;
    t->ni = w->n_intermediate;
    for (int k = 0; k < t->ni; ++k) t->inter_after[k] = w->intermediate[k];
    t->save_before = w->intermediate_save_point;
    t->eps = w->norm_eps;
    return MME_OK;
}

// every tensor of the checkpoint with its element count (the order of the staged bytes)
template <class Fn>
void each_tile_tensor(mme_tile_vit_weights& w, std::vector<mme_tile_layer>& layer, Fn&& f) {
    const size_t D = TD, F = TF;
    f(w.class_embedding, D);
    f(w.patch_w, D * TPDIM);
    f(w.pos_emb, (size_t)TTOK * D);
    f(w.tile_pos_emb, (size_t)TARATIOS * TTILES * TTOK * D);
    f(w.pre_emb, (size_t)TARATIOS * TTILES * D);
    f(w.post_emb, (size_t)TARATIOS * TTILES * D);
    f(w.ln_pre_g, D); f(w.ln_pre_b, D);
    f(w.ln_post_g, D); f(w.ln_post_b, D);
    for (mme_tile_layer& a : layer) {
        f(a.ln1_g, D); f(a.ln1_b, D);
        f(a.q_w, D * D); f(a.k_w, D * D); f(a.v_w, D * D); f(a.o_w, D * D);
        f(a.ln2_g, D); f(a.ln2_b, D);
        f(a.fc1_w, F * D); f(a.fc1_b, F);
        f(a.fc2_w, D * F); f(a.fc2_b, D);
    }
}

// The prepared buffers of the tower, in the order mme_weights_fingerprint reports them: nine tables, zeros, patch_w, then
// 9 per layer (o_b is the shared zeros table).  The tanh gates are applied here, once (tanh on the host): the kernels add plain tables.  A gated table
// and fc2_b are always multiplied, o_w / fc2_w only where the factor is not 1 (the ungated layers).
template <class P>
int prepare_tile(mme_ctx* c, P& p, const mme_tile_vit_weights& w) {
    TileVitDev* t = c->tv;
    int r;
    const size_t D = TD, F = TF;
    const size_t rD[3] = {D, D, D}, rF[1] = {F};
    auto plain = [&](const float* src, size_t n, float** dst) { return p.table(src, n, 1.f, false, dst); };
    const float g_pos = std::tanh(w.pos_gate), g_pre = std::tanh(w.pre_gate), g_post = std::tanh(w.post_gate);
    if ((r = plain(w.class_embedding, D, &t->cls))) return r;
    if ((r = p.table(w.pos_emb, (size_t)TTOK * D, 1.0f - g_pos, true, &t->pos))) return r;
    if ((r = p.table(w.tile_pos_emb, (size_t)TARATIOS * TTILES * TTOK * D, g_pos, true, &t->tilepos))) return r;
    if ((r = p.table(w.pre_emb, (size_t)TARATIOS * TTILES * D, g_pre, true, &t->pre))) return r;
    if ((r = p.table(w.post_emb, (size_t)TARATIOS * TTILES * D, g_post, true, &t->post))) return r;
    if ((r = plain(w.ln_pre_g, D, &t->lnpre_g))) return r;
    if ((r = plain(w.ln_pre_b, D, &t->lnpre_b))) return r;
    if ((r = plain(w.ln_post_g, D, &t->lnpost_g))) return r;
    if ((r = plain(w.ln_post_b, D, &t->lnpost_b))) return r;
    if ((r = p.zeros(F, &t->zeros))) return r;
    // patch projection [1280, 588] -> [1280, 640] (zero columns: the GEMM's K step is 64)
    if ((r = p.padded(w.patch_w, TD, TPDIM, TPDIMP, &t->patch_w))) return r;
    const int L = w.layers + w.global_layers;
    t->layer.resize(L);
    // The attention kernels take their scores in log2 units straight from the matrix pipe (attention_tiles.hip):
    // 80^-0.5 * log2(e) is folded into the query projection here, once, BEFORE the rounding to bf16 (as prepare_vit does)
    const float qsc = 0.11180339887498949f * 1.44269504088896341f;
    for (int l = 0; l < L; ++l) {
        const mme_tile_layer& a = w.layer[l];
        BlockW& Ld = t->layer[l];
        // x + tanh(gate) * branch(x): the gate multiplies the branch's LAST linear map (global layers only)
        const float ga = a.gated ? std::tanh(a.gate_attn) : 1.0f, gf = a.gated ? std::tanh(a.gate_ffn) : 1.0f;
        const WpFoldSrc fq[3] = {{a.q_w, nullptr, qsc, 1}, {a.k_w, nullptr, 1.f, 0}, {a.v_w, nullptr, 1.f, 0}};
        if ((r = p.folded(fq, rD, 3, D, a.ln1_g, a.ln1_b, &Ld.qkv_wf, &Ld.qkv_cs, &Ld.qkv_bf))) return r;
        const void *o_w = a.o_w, *fc2_w = a.fc2_w;
        if ((r = p.bf16(&o_w, rD, 1, D, ga, ga != 1.0f, &Ld.o_w))) return r;
        Ld.o_b = t->zeros;  // the checkpoint has no o_proj bias
        const WpFoldSrc f1[1] = {{a.fc1_w, a.fc1_b, 1.f, 0}};
        if ((r = p.folded(f1, rF, 1, D, a.ln2_g, a.ln2_b, &Ld.fc1_wf, &Ld.fc1_cs, &Ld.fc1_bf))) return r;
        if ((r = p.bf16(&fc2_w, rD, 1, F, gf, gf != 1.0f, &Ld.fc2_w))) return r;
        if ((r = p.table(a.fc2_b, D, gf, true, &Ld.fc2_b))) return r;
    }
    return MME_OK;
}

template <class P>
int load_tile(mme_ctx* c, const mme_tile_vit_weights* w, P p) {
    int r;
    if ((r = new_tile_dev(c, w))) return r;
    // the preparer's view of the tensors: the caller's pointers, or where the preparer staged them
    std::vector<mme_tile_layer> layer(w->layer, w->layer + w->layers + w->global_layers);
    mme_tile_vit_weights v = *w;
    v.layer = layer.data();
    r = p.stage([&](auto& put) { each_tile_tensor(v, layer, put); });
    if (r == MME_OK) r = prepare_tile(c, p, v);
    return p.finish(r);
}

}  // namespace

extern "C" {

int mme_load_tile_vit(mme_ctx* c, const mme_tile_vit_weights* w) {
    int r;
    if ((r = validate_tile_weights(c, w))) return r;
    return load_tile(c, w, HostPrep{c});
}

int mme_load_tile_vit_as(mme_ctx* c, const mme_tile_vit_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_tile_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_tile_vit_as"))) return r;
    return load_tile(c, w, DevPrep(c, dtype, stream, "mme_load_tile_vit_as"));
}

int mme_tile_vit_forward(mme_ctx* c, const float* pixel_values, const int32_t* aspect_ids_host, const int32_t* num_tiles_host, int n,
                         float* hidden, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    if (!c->tv) return fail(c, MME_E_STATE, "mme_tile_vit_forward: call mme_load_tile_vit first");
    if (n < 0 || (n > 0 && (!pixel_values || !aspect_ids_host || !num_tiles_host))) return fail(c, MME_E_ARG, "mme_tile_vit_forward: null argument or n<0");
    if (n == 0) return MME_OK;
    for (int i = 0; i < n; ++i)
        if (aspect_ids_host[i] < 1 || aspect_ids_host[i] >= TARATIOS || num_tiles_host[i] < 1 || num_tiles_host[i] > TTILES)
            return fail(c, MME_E_ARG, "mme_tile_vit_forward: image %d has aspect-ratio id %d / %d tiles (ids 1..8, tiles 1..4)", i, aspect_ids_host[i], num_tiles_host[i]);
    HIP_TRY(c, hipSetDevice(c->device));
    TileVitDev* t = c->tv;
    hipStream_t s = (hipStream_t)stream;
    // images per pass: the workspace is ~230 MB per image (qkv 49, mlp 66, five intermediate states 82, ...)
    const int per_pass = c->chunk >= 64 ? 64 : (c->chunk < 1 ? 1 : c->chunk);
    const int cap = n < per_pass ? n : per_pass;
    if (t->ws_images < cap) {
        const size_t rows = (size_t)cap * TT;
        int r;
        if ((r = ensure(c, t->patches, (size_t)cap * TTILES * TGRID * TGRID * TPDIMP * 2))) return r;
        if ((r = ensure(c, t->pemb, (size_t)cap * TTILES * TGRID * TGRID * TD * 2))) return r;
        if ((r = ensure(c, t->x, rows * TD * 2))) return r;
        if ((r = ensure(c, t->qkv, rows * 3 * TD * 2))) return r;
        if ((r = ensure(c, t->att, rows * TD * 2))) return r;
        if ((r = ensure(c, t->mlp, rows * TF * 2))) return r;
        if ((r = ensure(c, t->stats, rows * 2 * sizeof(float)))) return r;
        if ((r = ensure(c, t->lnpart, rows * 2 * (TD / 64) * sizeof(float)))) return r;
        if ((r = ensure(c, t->inter, (size_t)(t->ni > 0 ? t->ni : 1) * rows * TD * 2))) return r;
        if ((r = ensure(c, t->meta, (size_t)cap * 2 * sizeof(int32_t)))) return r;
        t->ws_images = cap;
    }
    const int64_t ws_rows = (int64_t)t->ws_images * TT;
    for (int i0 = 0; i0 < n; i0 += per_pass) {
        const int m = n - i0 < per_pass ? n - i0 : per_pass;
        const int M = m * TT;
        if (i0 > 0) HIP_TRY(c, hipStreamSynchronize(s));  // the id tables of successive passes share one device buffer
        int32_t* aid_dev = (int32_t*)t->meta.p;
        int32_t* nt_dev = aid_dev + t->ws_images;
        HIP_TRY(c, hipMemcpyAsync(aid_dev, aspect_ids_host + i0, (size_t)m * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(nt_dev, num_tiles_host + i0, (size_t)m * 4, hipMemcpyHostToDevice, s));
        const int L = t->layers + t->global_layers;
        int r;
        if ((r = reset_attn_guards(c, L, s))) return r;
        const int64_t npatch = (int64_t)m * TTILES * TGRID * TGRID;
        {
            Timed tm(c, s, KC_PRE);
            HIP_TRY(c, launch_tile_patchify(pixel_values + (size_t)i0 * TTILES * 3 * 560 * 560, t->patches.p, npatch, s));
        }
        EncoderPass P{c, s, TD, TF, t->eps, /*act: erf-GELU*/ 0, t->x.p, t->qkv.p, t->att.p, t->mlp.p, (float*)t->stats.p};
        P.lnpart = (float*)t->lnpart.p;  // handed to the residual GEMMs in every mode,
        P.lnpart_rows = ws_rows;
        P.planes = c->ln_mode == 2;      // used in mode 2: 1280 is a multiple of the 256-column tile
        P.zigzag = 0;                    // every kernel walks the rows forwards
        {
            GemmArgs g{};
            g.A = t->patches.p; g.W = t->patch_w; g.M = (int)npatch; g.N = TD; g.K = TPDIMP; g.bias = t->zeros; g.out = t->pemb.p; g.ldo = TD;
            if ((r = P.gemm(EPI_BIAS, g))) return r;
        }
        {
            Timed tm(c, s, KC_LN);
            HIP_TRY(c, launch_tile_assemble(t->pemb.p, t->cls, t->pre, t->pos, t->tilepos, t->lnpre_g, t->lnpre_b, aid_dev, t->x.p, M, 1e-5f, s));
        }
        if ((r = P.stats_from_x(t->x.p, 0, M))) return r;
        int saved = 0;
        for (int l = 0; l < L; ++l) {
            // an intermediate state the output concatenates, "before layer l" convention: the state ENTERING local layer l
            if (t->save_before && l < t->layers && saved < t->ni && t->inter_after[saved] == l) {
                HIP_TRY(c, hipMemcpyAsync((char*)t->inter.p + (size_t)saved * ws_rows * TD * 2, t->x.p, (size_t)M * TD * 2, hipMemcpyDeviceToDevice, s));
                ++saved;
            }
            if (l == t->layers) {  // between the local and the global stack: layernorm_post + post-tile embedding
                {
                    Timed tm(c, s, KC_LN);
                    HIP_TRY(c, launch_tile_ln_post(t->x.p, t->lnpost_g, t->lnpost_b, t->post, aid_dev, M, 1e-5f, s));
                }
                if ((r = P.stats_from_x(t->x.p, 0, M))) return r;
            }
            if ((r = P.qkv_ln(t->layer[l], M, 3 * TD))) return r;
            {
                Timed tm(c, s, KC_ATTN);
                HIP_TRY(c, launch_attention_tiles(t->qkv.p, t->att.p, nt_dev, m, s, c->attn_mode ? (int*)c->attn_guard.p + l : nullptr, c->attn_mode == 2));
            }
            // statistics are needed by the next layer's QKV GEMM, except after the last local layer (layernorm_post
            // rewrites x first) and after the very last layer: there fc2 takes the plain EPI_BIAS_RES epilogue
            const bool need_stats = l + 1 < L && l + 1 != t->layers;
            if ((r = P.after_attention(t->layer[l], M, t->att.p, t->x.p, need_stats))) return r;
            if (!t->save_before && l < t->layers && saved < t->ni && t->inter_after[saved] == l) {  // "after layer l" convention
                HIP_TRY(c, hipMemcpyAsync((char*)t->inter.p + (size_t)saved * ws_rows * TD * 2, t->x.p, (size_t)M * TD * 2, hipMemcpyDeviceToDevice, s));
                ++saved;
            }
        }
        Timed tm(c, s, KC_POOL);
        const int F = TD * (1 + t->ni);
        if (hidden)
            HIP_TRY(c, launch_tile_output(t->x.p, t->inter.p, t->ni, ws_rows * TD, hidden + (size_t)i0 * TTILES * TTOK * F, (int64_t)m * TTILES * TTOK, s));
        if (emb_f32 || emb_bf16)
            HIP_TRY(c, launch_tile_pool(t->x.p, t->inter.p, t->ni, ws_rows * TD, m, emb_f32 ? emb_f32 + (size_t)i0 * F : nullptr,
                                        emb_bf16 ? (void*)(emb_bf16 + (size_t)i0 * F) : nullptr, s));
    }
    return MME_OK;
}

// ---- single launches of the row kernels on caller-owned buffers (tests/test_gpu_tile_rows.py): as mme_rowop_apply, every
// assumption of the kernels is checked here, so that a bad argument is an MME_E_ARG and never a launch
int mme_tile_rowop_apply(mme_ctx* c, int op, const mme_tile_rowop_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_tile_rowop_apply", a, op, 4)) return r;
    const int64_t count_max = 0x7fffffff;
    const int64_t count = op == 0 ? a->npatch : op == 3 ? a->out_rows : op == 4 ? (int64_t)a->n : a->rows;
    const char* bad = nullptr;
    int64_t last_row = 0;  // ops 3, 4: the last row of x and of every state the launch reads
    switch (op) {
        case 0:
            if (!vec16(a->pv) || !vec16(a->patches)) bad = "pv, patches non-null and 16-byte aligned";
            else if (count < 0 || count > count_max) bad = "0 <= npatch <= 2^31 - 1";
            break;
        case 1:
            if (!vec16(a->pemb) || !vec16(a->cls) || !vec16(a->pre) || !vec16(a->pos) || !vec16(a->tilepos) || !vec16(a->gamma) || !vec16(a->beta) || !vec16(a->x))
                bad = "pemb, cls, pre, pos, tilepos, gamma, beta, x non-null and 16-byte aligned";
            break;
        case 2:
            if (!vec16(a->x) || !vec16(a->gamma) || !vec16(a->beta) || !vec16(a->post)) bad = "x, gamma, beta, post non-null and 16-byte aligned";
            break;
        case 3:
            if (!vec16(a->x) || !vec16(a->hidden)) bad = "x, hidden non-null and 16-byte aligned";
            else if (count < 0 || count > count_max) bad = "0 <= out_rows <= 2^31 - 1";
            else if (count > 0) last_row = (count - 1) / TTOK * TTOKP + (count - 1) % TTOK;
            break;
        default:
            if (!vec16(a->x)) bad = "x non-null and 16-byte aligned";
            else if (!a->emb_f32 && !a->emb_bf16) bad = "emb_f32 or emb_bf16";
            else if (((uintptr_t)a->emb_f32 & 15) || ((uintptr_t)a->emb_bf16 & 15)) bad = "emb_f32 and emb_bf16 16-byte aligned";
            else if (count < 0) bad = "n >= 0";
            else if (count > 0) last_row = (count - 1) * TT;
            break;
    }
    if (!bad && (op == 1 || op == 2)) {
        if (!a->aid || ((uintptr_t)a->aid & 3)) bad = "aid non-null and 4-byte aligned";
        else if (count < 0 || count > count_max) bad = "0 <= rows <= 2^31 - 1";
        else if (a->aspect_rows < 1 || a->aspect_rows > TARATIOS) bad = "aspect_rows in 1..9";
    }
    if (!bad && (op == 3 || op == 4)) {
        if (a->ni < 0 || a->ni > TMAXI) bad = "ni in 0..8";
        else if ((a->ni == 0) != (a->inter == nullptr)) bad = "inter null exactly when ni == 0";
        else if (a->inter && !vec16(a->inter)) bad = "inter 16-byte aligned";
        else if (a->ni > 1 && (a->inter_stride < (last_row + 1) * TD || a->inter_stride > ((int64_t)1 << 40)))
            bad = "inter_stride >= the elements of one state ((last source row + 1) * 1280) and <= 2^40";
    }
    if (bad) return fail(c, MME_E_ARG, "mme_tile_rowop_apply: op %d needs %s", op, bad);
    if (count == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (op == 1 || op == 2) {  // the kernels index the caller's tables by these values
        std::vector<int32_t> ids((size_t)((count + TT - 1) / TT));
        HIP_TRY(c, hipMemcpyAsync(ids.data(), a->aid, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < ids.size(); ++i)
            if (ids[i] < 0 || ids[i] >= a->aspect_rows)
                return fail(c, MME_E_ARG, "mme_tile_rowop_apply: aid[%lld] = %d outside 0..%d (aspect_rows - 1)", (long long)i, ids[i], a->aspect_rows - 1);
    }
    switch (op) {
        case 0: HIP_TRY(c, launch_tile_patchify(a->pv, a->patches, a->npatch, s)); break;
        case 1: HIP_TRY(c, launch_tile_assemble(a->pemb, a->cls, a->pre, a->pos, a->tilepos, a->gamma, a->beta, a->aid, a->x, a->rows, a->eps, s)); break;
        case 2: HIP_TRY(c, launch_tile_ln_post(a->x, a->gamma, a->beta, a->post, a->aid, a->rows, a->eps, s)); break;
        case 3: HIP_TRY(c, launch_tile_output(a->x, a->inter, a->ni, a->inter_stride, a->hidden, a->out_rows, s)); break;
        default: HIP_TRY(c, launch_tile_pool(a->x, a->inter, a->ni, a->inter_stride, a->n, a->emb_f32, a->emb_bf16, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // extern "C"
