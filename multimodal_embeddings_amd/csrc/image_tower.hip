// The image towers (ViT, CLIP, SigLIP, DINOv2 at 224 pixels): one pass as stem, blocks and tail over the shared block of
// encoder_pass.h, one chunk driver, and the five entry points that feed it (include/mme.h).  K1 itself is capi.hip's.
#include "encoder_pass.h"

namespace {

// bf16 values of one crop's patch matrix as K1 writes it: 196 x 768 = 49 x 3072
constexpr size_t CROP_VALUES = (size_t)VIT_NP * VIT_PATCH_DIM;

// The workspace follows the chunk AND the geometry: a context that was reloaded with a wider encoder regrows it
// (ensure() never shrinks a buffer, so going back to a narrower one keeps what is there).
int ensure_workspace(mme_ctx* c) {
    const int D = c->geom.hidden, F = c->geom.mlp;
    const int T = c->geom.tokens();  // 197, or 50 at patch 32 (a quarter of the rows; ensure() keeps the larger buffers)
    if (c->ws_chunk == c->chunk && c->ws_hidden == D && c->ws_mlp == F && c->ws_tokens == T) return MME_OK;
    const size_t rows = (size_t)c->chunk * T;
    int r;
    if ((r = ensure(c, c->x, rows * D * 2))) return r;
    if ((r = ensure(c, c->hbuf, rows * D * 2))) return r;
    if ((r = ensure(c, c->qkv, rows * 3 * D * 2))) return r;
    if ((r = ensure(c, c->att, rows * D * 2))) return r;
    if ((r = ensure(c, c->mlp, rows * F * 2))) return r;
    if ((r = ensure(c, c->stats, rows * 2 * sizeof(float)))) return r;
    if ((r = ensure(c, c->lnpart, rows * 2 * (D / 64) * sizeof(float)))) return r;
    c->ws_chunk = c->chunk;
    c->ws_hidden = D;
    c->ws_mlp = F;
    c->ws_tokens = T;
    return MME_OK;
}

// What one pass is asked for; the chunk driver moves the three outputs on per chunk.
struct PassOut {
    int pool_token;
    float* emb_f32;    // [n, embed_dim], either may be null
    bf16_t* emb_bf16;
    // mme_vit_tokens / mme_embed_tokens: the final LayerNorm + L2 of rows tok0 .. tok0 + ntok - 1 of every crop go to
    // tokens bf16 [n, ntok, hidden], and the last block runs unpruned whatever prune_last says
    bf16_t* tokens = nullptr;
    int tok0 = 0, ntok = 0;
    // mme_set_pooling (forward_chunks fills both in): under MME_POOL_MEAN / MME_POOL_CLS_MEAN the tail averages the patch rows of
    // every crop's covered grid -- grids: DEVICE int32 [n, 2] of the chunk, null = whole grids -- pool_token is not read, and
    // the last block runs unpruned as for a token pass
    int pool_mode = MME_POOL_TOKEN;
    const int32_t* grids = nullptr;
};

// Patch embedding and token rows into x, the guard reset, and the first LayerNorm statistics of the pass (those of every
// later one come from the block: EncoderPass::stats_after).
int stem(EncoderPass& P, const bf16_t* patches, int n) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    const VitGeom& G = c->geom;
    const int D = P.D, M = n * G.tokens();
    // Patch 16 with a class token: EPI_PATCH adds bias and position rows and maps patch rows past the [CLS] rows at
    // compile time.  Every other tower (patch 32, patch 14; SigLIP, whose patch row m IS token row m) leaves f32
    // [n * np, D] in the qkv buffer, dead until layer 0, and a row kernel adds bias and position rows in EPI_PATCH's f32
    // order, rounds once and writes the [CLS] rows, where there are any, in the same launch.
    const bool fused = !G.layout().embed_rows;
    GemmArgs g{};
    g.A = patches; g.W = c->patch_w; g.M = n * G.np(); g.N = D; g.K = G.patch_dim();
    int r;
    if (fused) {
        g.bias = c->patch_b; g.pos = c->pos; g.out = c->x.p; g.ldo = D;
        if (P.planes && !c->clip) {  // the 256 x 256 kernel leaves the LayerNorm partial sums of the token rows it writes
            g.ln_part = P.lnpart;
            g.ln_part_rows = P.lnpart_rows;
        }
        if ((r = P.gemm(EPI_PATCH, g))) return r;
        Timed t(c, s, KC_LN);
        HIP_TRY(c, launch_cls_rows(c->x.p, c->cls, c->pos, n, D, s));
    } else {
        g.outf = (float*)c->qkv.p; g.ldf = D;
        if ((r = P.gemm(EPI_F32, g))) return r;
        Timed t(c, s, KC_LN);
        HIP_TRY(c, launch_embed_rows(g.outf, c->patch_b, c->pos, G.no_cls ? nullptr : c->cls, c->x.p, n, G.tokens(), D, s));
    }
    if ((r = reset_attn_guards(c, G.layers, s))) return r;
    if (c->clip) {
        // CLIP: pre_layrnorm over every token row, in place; the same launch leaves the statistics of the rows it wrote,
        // in the canonical order: the first folded LayerNorm needs neither planes nor another pass over x
        Timed t(c, s, KC_LN);
        HIP_TRY(c, launch_pre_ln(c->x.p, c->pre_g, c->pre_b, M, D, c->ln_eps, P.stats, s));
    } else if (fused && P.planes && gemm_runs_256(g, c->gemm_variant)) {  // (no planes from the f32 epilogue; the canonical pass below gives the same bits)
        // the patch-embed epilogue left the partial sums of every token row an INTERIOR tile wrote (patch rows
        // [0, interior) -> token rows up to t_int); the [CLS] rows (written by cls_rows, every 197th row) and the rows
        // of the ragged last tile take the stand-alone kernel, same canonical order
        const int64_t interior = gemm_interior_rows(EPI_PATCH, g, c->gemm_variant);        // patch rows
        const int64_t t_int = interior ? interior - 1 + (interior - 1) / VIT_NP + 2 : 0;   // one past the last token row they map to
        Timed t(c, s, KC_LN);
        HIP_TRY(c, launch_ln_finish(P.lnpart, P.lnpart_rows, t_int, D, c->ln_eps, P.stats, s));
        HIP_TRY(c, launch_ln_stats_canonical(c->x.p, 0, t_int, D, c->ln_eps, P.stats, s, VIT_T));  // [CLS] rows below t_int
        HIP_TRY(c, launch_ln_stats_canonical(c->x.p, t_int, M, D, c->ln_eps, P.stats, s));
    } else if (!P.unfolded()) {
        return P.stats_from_x(c->x.p, 0, M);
    }
    return MME_OK;
}

// Pruned last layer (mme_set_forward_pruning): after the last attention only ONE token row per crop is ever read (K8
// pools token `pool_token`), so the query block that holds it is the only one attended, and the second half of the
// block runs on the n gathered rows instead of n x 197.  Same kernels, same per-row arithmetic: the embeddings are
// bit-identical to the full pass (tests/test_gpu_parity.py).
int second_half_on_pool_rows(EncoderPass& P, const LayerDev& L, int n, int pool_token) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    bf16_t* att_p = (bf16_t*)c->hbuf.p;         // [n, D] gathered attention rows
    bf16_t* x_p = att_p + (size_t)n * P.D;      // [n, D] gathered residual rows (hbuf holds rows x D: n x 197 of them)
    const size_t rowb = (size_t)P.D * 2, pitch = (size_t)c->geom.tokens() * rowb;
    {
        Timed t(c, s, KC_POOL);
        HIP_TRY(c, hipMemcpy2DAsync(att_p, rowb, (const char*)c->att.p + (size_t)pool_token * rowb, pitch, rowb, n, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpy2DAsync(x_p, rowb, (const char*)c->x.p + (size_t)pool_token * rowb, pitch, rowb, n, hipMemcpyDeviceToDevice, s));
    }
    int r;
    if ((r = P.on_few_rows().second_half(L, n, att_p, x_p, false))) return r;
    Timed t(c, s, KC_POOL);  // back into the residual stream, where the pooling kernel reads the row
    HIP_TRY(c, hipMemcpy2DAsync((char*)c->x.p + (size_t)pool_token * rowb, pitch, x_p, rowb, rowb, n, hipMemcpyDeviceToDevice, s));
    return MME_OK;
}

int blocks(EncoderPass& P, int n, const PassOut& o) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    const VitGeom& G = c->geom;
    const int T = G.tokens(), M = n * T;
    int r;
    for (int l = 0; l < G.layers; ++l) {
        const LayerDev& L = c->layer[l];
        const bool last = l + 1 == G.layers;
        if ((r = P.first_half(L, L.ln1_g, L.ln1_b, M, 3 * P.D))) return r;
        // (the unfolded form, SigLIP's head, a token pass and mean pooling read every token row)
        const bool pruned = c->prune_last && last && !P.unfolded() && !c->siglip && !o.tokens && o.pool_mode == MME_POOL_TOKEN;
        const int only_block = pruned ? o.pool_token / 32 : -1;
        {
            Timed t(c, s, KC_ATTN);
            if (G.layout().attn != ATTN_LONG) {  // exact kernels only: the guard words stay zero; the walk order is not taken (next_dir keeps the GEMMs' alternation)
                if (P.zigzag != 2) P.next_dir();
                HIP_TRY(c, launch_attention_exact(c->qkv.p, c->att.p, n, T, false, G.heads, s, only_block));
            } else {
                HIP_TRY(c, launch_attention(c->qkv.p, c->att.p, n, G.heads, s, c->attn_mode ? (int*)c->attn_guard.p + l : nullptr, c->attn_mode == 2,
                                            only_block, P.zigzag == 2 ? true : P.next_dir() != 0, T));
            }
        }
        // no statistics after the last block: the final LayerNorm touches the pooled row only (K8).  SigLIP:
        // post_layernorm, folded into the head's K | V GEMM, reads them
        if (pruned) r = second_half_on_pool_rows(P, L, n, o.pool_token);
        else r = P.second_half(L, M, c->att.p, c->x.p, !last || c->siglip);
        if (r) return r;
    }
    return MME_OK;
}

// SiglipMultiheadAttentionPoolingHead: K | V = in_proj(post_layernorm(x)) over every token row, one constant query per
// head (map_pool), then the second half of a block with the head's weights on n rows: out_proj on a ZEROED residual
// (0 + out_proj(a) is out_proj(a) in bf16: the probe is no residual), y = a' + fc2(act(fc1(LN(a')))); L2
int siglip_head(EncoderPass& P, int n, const PassOut& o) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    const int D = P.D;
    int r;
    if ((r = ensure(c, c->pooled, (size_t)2 * c->chunk * D * 2))) return r;
    bf16_t* a_p = (bf16_t*)c->pooled.p;   // [n, D] pooled attention rows
    bf16_t* y_p = a_p + (size_t)n * D;    // [n, D] the head's residual rows
    if ((r = P.first_half(c->head, c->lnf_g, c->lnf_b, n * c->geom.tokens(), 2 * D))) return r;
    {
        Timed t(c, s, KC_POOL);
        HIP_TRY(c, launch_map_pool(c->qkv.p, c->head_q, a_p, n, c->geom.heads, s));
        HIP_TRY(c, hipMemsetAsync(y_p, 0, (size_t)n * D * 2, s));
    }
    if ((r = P.on_few_rows().second_half(c->head, n, a_p, y_p, false))) return r;
    Timed t(c, s, KC_POOL);
    HIP_TRY(c, launch_l2_rows_bf16(y_p, n, D, o.emb_f32, o.emb_bf16, s));
    return MME_OK;
}

// CLIP with a projection: post_layernorm of the pooled row, rounded to bf16, times visual_projection, then L2
int clip_projection(EncoderPass& P, int n, const PassOut& o) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    const int D = P.D, E = c->proj_dim;
    int r;
    if ((r = ensure(c, c->pooled, (size_t)c->chunk * D * 2))) return r;
    if ((r = ensure(c, c->projf, (size_t)c->chunk * E * sizeof(float)))) return r;
    {
        Timed t(c, s, KC_POOL);
        HIP_TRY(c, launch_pool_ln(c->x.p, c->lnf_g, c->lnf_b, n, c->geom.tokens(), o.pool_token, D, c->ln_eps, c->pooled.p, s));
    }
    GemmArgs g{};
    g.A = c->pooled.p; g.W = c->proj_w; g.M = n; g.N = E; g.K = D;
    g.outf = (float*)c->projf.p; g.ldf = E;
    if ((r = P.gemm(EPI_F32, g))) return r;
    Timed t(c, s, KC_POOL);
    HIP_TRY(c, launch_l2_rows(g.outf, n, E, o.emb_f32, o.emb_bf16, s));
    return MME_OK;
}

int tail(EncoderPass& P, int n, const PassOut& o) {
    mme_ctx* c = P.c;
    hipStream_t s = P.s;
    const int D = P.D, T = c->geom.tokens();
    if (o.tokens) {  // the token rows of the last block, before any tail touches the workspace (none writes x)
        Timed t(c, s, KC_POOL);
        HIP_TRY(c, launch_token_rows(c->x.p, c->lnf_g, c->lnf_b, n, T, o.tok0, o.ntok, D, c->ln_eps, o.tokens, s));
    }
    if (c->siglip) return siglip_head(P, n, o);
    if (c->proj_dim) return clip_projection(P, n, o);
    Timed t(c, s, KC_POOL);
    if (o.pool_mode != MME_POOL_TOKEN)
        HIP_TRY(c, launch_pool_mean(c->x.p, c->lnf_g, c->lnf_b, o.grids, n, T, VIT_IMG / c->geom.patch, 1, o.pool_mode == MME_POOL_CLS_MEAN, D, c->ln_eps,
                                    o.emb_f32, o.emb_bf16, s));
    else
        HIP_TRY(c, launch_pool(c->x.p, c->lnf_g, c->lnf_b, n, T, o.pool_token, D, c->ln_eps, o.emb_f32, o.emb_bf16, s));
    return MME_OK;
}

// One pass over n <= chunk crops.  What a tower sets: the geometry (VitGeom), pre-LN and projection (CLIP), the
// activation, the head (SigLIP); what the caller sets: ln_mode, tile order, attention mode, pruning.
int forward_chunk(mme_ctx* c, const bf16_t* patches, int n, const PassOut& o, hipStream_t s) {
    const int D = c->geom.hidden;
    EncoderPass P{c, s, D, c->geom.mlp, c->ln_eps, c->act, c->x.p, c->qkv.p, c->att.p, c->mlp.p, (float*)c->stats.p};
    P.hbuf = c->ln_mode == 0 ? c->hbuf.p : nullptr;
    P.lnpart = (float*)c->lnpart.p;  // handed to the residual GEMMs in every mode,
    P.lnpart_rows = (int64_t)c->ws_chunk * c->geom.tokens();
    // used where the epilogues leave all of them: they leave the partial planes from their interior-tile code only, and
    // at a width that is no multiple of the 256-column tile (384) the last column tile of every row panel is no interior
    // tile: its two slices would be missing.  There mode 2 takes mode 1's statistics pass over x, which sums in the same
    // canonical order: the same bits, one more read of x per LayerNorm.
    P.planes = c->ln_mode == 2 && (D % 256) == 0;
    P.zigzag = c->zigzag;  // mme_set_tile_order; only this tower alternates the walk (the patch embedding and the tails walk forwards)
    int r;
    if ((r = stem(P, patches, n))) return r;
    if ((r = blocks(P, n, o))) return r;
    return tail(P, n, o);
}

// K1 of m <= chunk crops into `dst` in the tower's patch layout.  Patch 16: K1 writes it.  Patch 32 / 14: K1 writes its
// patch-16 matrix into the staging buffer of one chunk (c->patches) and the retile kernel permutes it into dst
// [m * 49, 3072] (the same bytes per crop) or [m * 256, 640].
int patches_chunk(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int m, bf16_t* dst, hipStream_t s) {
    const bool retile = c->geom.patch != VIT_PATCH;
    int r;
    if ((r = preprocess_chunk(c, pix, offs, hw, m, retile ? (bf16_t*)c->patches.p : dst, s))) return r;
    if (!retile) return MME_OK;
    Timed t(c, s, KC_PRE);
    HIP_TRY(c, launch_retile(c->geom.patch, c->patches.p, dst, m, s));
    return MME_OK;
}

// The buffers of the pixel path (mme_embed, mme_embed_tokens): the workspace, K1's staging buffer, the retiled matrix (ensure() only grows it)
int ensure_pixel_path(mme_ctx* c) {
    int r;
    if ((r = ensure_workspace(c))) return r;
    if ((r = ensure(c, c->patches, (size_t)c->chunk * CROP_VALUES * 2))) return r;
    if (c->geom.patch != VIT_PATCH && (r = ensure(c, c->retiled, (size_t)c->chunk * c->geom.crop_values() * 2))) return r;
    return MME_OK;
}

// The chunk loop of the four forward entry points.  pix null: `patches` holds the n crops' patch matrices.  Else every
// chunk is preprocessed first (K1 -> retile -> pass), behind a synchronise: the crop tables of successive chunks reuse
// one device buffer.  Under mme_set_pooling's mean modes the covered grids go to the device in c->pool_grids: those of a patch
// call (`grids`: host int32 [n, 2], validated by the caller; null = whole grids, nothing is copied) once, those of the pixel
// path (pool_grids_host over the chunk's crop sizes) per chunk behind the same synchronise.
int forward_chunks(mme_ctx* c, const bf16_t* patches, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, PassOut all, hipStream_t s,
                   const int32_t* grids = nullptr) {
    bf16_t* staged = (bf16_t*)(c->geom.patch != VIT_PATCH ? c->retiled.p : c->patches.p);
    const size_t E = embed_dim(c), tok_values = (size_t)all.ntok * c->geom.hidden;
    all.pool_mode = c->pool_mode;
    const bool mean = all.pool_mode != MME_POOL_TOKEN;
    int r;
    if (mean && (pix || grids)) {
        if ((r = ensure(c, c->pool_grids, (size_t)(pix && n > c->chunk ? c->chunk : n) * 2 * sizeof(int32_t)))) return r;
        if (!pix) HIP_TRY(c, hipMemcpyAsync(c->pool_grids.p, grids, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    for (int s0 = 0; s0 < n; s0 += c->chunk) {
        const int m = n - s0 < c->chunk ? n - s0 : c->chunk;
        if (pix) {
            if (s0 > 0) HIP_TRY(c, hipStreamSynchronize(s));
            if ((r = patches_chunk(c, pix, offs + s0, hw + 2 * s0, m, staged, s))) return r;
            if (mean) {
                c->h_pool_grids.resize((size_t)2 * m);
                if ((r = pool_grids_host(c, "mme_embed", hw + 2 * s0, m, c->h_pool_grids.data()))) return r;
                // a pageable-host copy, staged before the call returns: the vector is free for the next chunk
                HIP_TRY(c, hipMemcpyAsync(c->pool_grids.p, c->h_pool_grids.data(), (size_t)m * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            }
        }
        PassOut o = all;
        if (mean && (pix || grids)) o.grids = (const int32_t*)c->pool_grids.p + (pix ? 0 : (size_t)2 * s0);
        if (o.emb_f32) o.emb_f32 += s0 * E;
        if (o.emb_bf16) o.emb_bf16 += s0 * E;
        if (o.tokens) o.tokens += s0 * tok_values;
        if ((r = forward_chunk(c, pix ? staged : patches + s0 * c->geom.crop_values(), m, o, s))) return r;
    }
    return MME_OK;
}

// what mme_vit_tokens / mme_embed_tokens refuse alike
int check_token_call(mme_ctx* c, const char* who, int pool_token, int tok0, int ntok, const void* tokens) {
    if (!c->loaded && c->tv) return fail(c, MME_E_STATE, "%s: encoder tile_vit; supported: the single-tile image towers (vit, clip, siglip, dinov2)", who);
    if (!c->loaded) return fail(c, MME_E_STATE, "%s: call mme_load_vit first", who);
    const int T = c->geom.tokens();
    if (pool_token < 0 || pool_token >= T) return fail(c, MME_E_ARG, "%s: pool_token %d outside 0..%d", who, pool_token, T - 1);
    if (tok0 < 0 || ntok < 1 || (int64_t)tok0 + ntok > T)
        return fail(c, MME_E_ARG, "%s: token window tok0 %d, ntok %d; supported tok0 >= 0, ntok >= 1, tok0 + ntok <= %d (the tower's tokens)", who, tok0, ntok, T);
    if (!tokens) return fail(c, MME_E_ARG, "%s: tokens_bf16_dev is NULL", who);
    return MME_OK;
}

}  // namespace

extern "C" {

int mme_preprocess(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, uint16_t* patches, void* stream) {
    if (!c) return MME_E_ARG;
    if (n < 0 || (n > 0 && (!pix || !offs || !hw || !patches))) return fail(c, MME_E_ARG, "mme_preprocess: null argument or n<0");
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (c->geom.patch != VIT_PATCH && (r = ensure(c, c->patches, (size_t)c->chunk * CROP_VALUES * 2))) return r;
    // the crop tables of successive chunks reuse one device buffer: chunk so that stays ordered
    for (int s0 = 0; s0 < n; s0 += c->chunk) {
        const int m = n - s0 < c->chunk ? n - s0 : c->chunk;
        if (s0 > 0) HIP_TRY(c, hipStreamSynchronize(s));
        if ((r = patches_chunk(c, pix, offs + s0, hw + 2 * s0, m, (bf16_t*)patches + (size_t)s0 * c->geom.crop_values(), s))) return r;
    }
    return MME_OK;
}

int mme_vit_forward(mme_ctx* c, const uint16_t* patches, int n, int pool_token, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    if (!c->loaded) return fail(c, MME_E_STATE, "mme_vit_forward: call mme_load_vit first");
    if (n < 0 || (n > 0 && !patches)) return fail(c, MME_E_ARG, "mme_vit_forward: null patches or n<0");
    if (pool_token < 0 || pool_token >= c->geom.tokens()) return fail(c, MME_E_ARG, "mme_vit_forward: pool_token %d outside 0..%d", pool_token, c->geom.tokens() - 1);
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = ensure_workspace(c);
    if (r) return r;
    return forward_chunks(c, (const bf16_t*)patches, nullptr, nullptr, nullptr, n, PassOut{pool_token, emb_f32, (bf16_t*)emb_bf16}, (hipStream_t)stream);
}

int mme_vit_forward_grids(mme_ctx* c, const uint16_t* patches, int n, const int32_t* grids, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    if (!c->loaded) return fail(c, MME_E_STATE, "mme_vit_forward_grids: call mme_load_vit first");
    if (c->pool_mode == MME_POOL_TOKEN)
        return fail(c, MME_E_STATE, "mme_vit_forward_grids: pooling mode %d (MME_POOL_TOKEN); supported: %d (MME_POOL_MEAN) and %d (MME_POOL_CLS_MEAN), see mme_set_pooling",
                    MME_POOL_TOKEN, MME_POOL_MEAN, MME_POOL_CLS_MEAN);
    if (n < 0 || (n > 0 && !patches)) return fail(c, MME_E_ARG, "mme_vit_forward_grids: null patches or n<0");
    const int g = VIT_IMG / c->geom.patch;
    for (int i = 0; grids && i < 2 * n; ++i)
        if (grids[i] < 1 || grids[i] > g)
            return fail(c, MME_E_ARG, "mme_vit_forward_grids: grids[%d][%d] = %d; supported 1..%d (the %d x %d patch grid)", i / 2, i % 2, grids[i], g, g, g);
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = ensure_workspace(c);
    if (r) return r;
    return forward_chunks(c, (const bf16_t*)patches, nullptr, nullptr, nullptr, n, PassOut{0, emb_f32, (bf16_t*)emb_bf16}, (hipStream_t)stream, grids);
}

int mme_embed(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, int pool_token, float* emb_f32,
              uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    if (!c->loaded) return fail(c, MME_E_STATE, "mme_embed: call mme_load_vit first");
    if (n < 0 || (n > 0 && (!pix || !offs || !hw))) return fail(c, MME_E_ARG, "mme_embed: null argument or n<0");
    if (pool_token < 0 || pool_token >= c->geom.tokens()) return fail(c, MME_E_ARG, "mme_embed: pool_token %d outside 0..%d", pool_token, c->geom.tokens() - 1);
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = ensure_pixel_path(c);
    if (r) return r;
    return forward_chunks(c, nullptr, pix, offs, hw, n, PassOut{pool_token, emb_f32, (bf16_t*)emb_bf16}, (hipStream_t)stream);
}

int mme_vit_tokens(mme_ctx* c, const uint16_t* patches, int n, int pool_token, int tok0, int ntok, uint16_t* tokens, float* emb_f32,
                   uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    int r = check_token_call(c, "mme_vit_tokens", pool_token, tok0, ntok, tokens);
    if (r) return r;
    if (n < 0 || (n > 0 && !patches)) return fail(c, MME_E_ARG, "mme_vit_tokens: null patches or n<0");
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = ensure_workspace(c))) return r;
    return forward_chunks(c, (const bf16_t*)patches, nullptr, nullptr, nullptr, n, PassOut{pool_token, emb_f32, (bf16_t*)emb_bf16, (bf16_t*)tokens, tok0, ntok},
                          (hipStream_t)stream);
}

int mme_embed_tokens(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, int pool_token, int tok0, int ntok,
                     uint16_t* tokens, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    int r = check_token_call(c, "mme_embed_tokens", pool_token, tok0, ntok, tokens);
    if (r) return r;
    if (n < 0 || (n > 0 && (!pix || !offs || !hw))) return fail(c, MME_E_ARG, "mme_embed_tokens: null argument or n<0");
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = ensure_pixel_path(c))) return r;
    return forward_chunks(c, nullptr, pix, offs, hw, n, PassOut{pool_token, emb_f32, (bf16_t*)emb_bf16, (bf16_t*)tokens, tok0, ntok}, (hipStream_t)stream);
}

}  // extern "C"
