// C ABI of the text towers (include/mme.h, "CLIP text tower" and "SigLIP text tower"): transformers' CLIPTextTransformer +
// text_projection, and SiglipTextTransformer with its head, on the GEMM, LayerNorm-folding and statistics machinery of the
// image path, with their own row kernels (text_tower.hip) and short-sequence attention kernels (attention_short.hip).  ONE
// record (TextDev), ONE prepare sequence and ONE pass serve both: the towers differ in the settings below (token count, mask,
// pooling rule, head bias).  The tower lives beside the context's image tower: its record and its workspace are here, its
// prepared buffers in c->allocs[text_alloc_lo, text_alloc_hi); a load of either kind replaces the other.
#include <cstring>
#include <new>
#include <vector>

#include "encoder_pass.h"

enum TextKind { TEXT_CLIP = 1, TEXT_SIGLIP = 2 };  // mme_text_geometry's first word

struct TextDev {
    bool loaded = false;
    int kind = TEXT_CLIP;
    int hidden = 0, layers = 0, heads = 0, mlp = 0, vocab = 0, proj_dim = 0, act = 0, eos = 0;
    int tokens = TXT_T;     // positions per sequence: 77 (CLIP) or 64 (SigLIP)
    bool causal = true;     // CLIP's causal mask; SigLIP attends every position, padding included
    bool pool_last = false; // pool position tokens - 1 of every sequence (SigLIP) instead of the EOS position (CLIP)
    int pad = 0;            // SigLIP's pad_token_id (== eos: the last word of mme_text_info)
    bool has_logits = false;
    float logit_scale = 0.f, logit_bias = 0.f;
    float eps = 1e-5f;
    bf16_t* tok = nullptr;
    float *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    bf16_t* proj_w = nullptr;
    float* proj_b = nullptr;  // SigLIP's head.bias [proj_dim]; null: a bias-free projection (CLIP)
    std::vector<BlockW> layer;
    // workspace of the pass (grown to the largest chunk seen, never shrunk), and the diagnostic's staging of ids / positions
    DevBuf x, qkv, att, hmlp, stats, pooled, projf, ids, eos_pos, apply_ints;
};

void text_free(mme_ctx* c) {
    if (!c->text) return;
    TextDev* t = c->text;
    DevBuf* bufs[] = {&t->x, &t->qkv, &t->att, &t->hmlp, &t->stats, &t->pooled, &t->projf, &t->ids, &t->eos_pos, &t->apply_ints};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    delete t;
    c->text = nullptr;
}

namespace {

int text_dev(mme_ctx* c, const char* who) {
    if (c->text) return MME_OK;
    c->text = new (std::nothrow) TextDev();
    if (!c->text) return fail(c, MME_E_NOMEM, "%s: out of host memory", who);
    return MME_OK;
}

int text_embed_dim(const TextDev* t) { return t->proj_dim ? t->proj_dim : t->hidden; }

// What the ONE load sequence reads: either public struct, restated.
struct TextW {
    int kind, hidden, layers, heads, mlp, vocab, tokens, proj_dim, act, eos;
    float ln_eps;
    bool has_logits;
    float logit_scale, logit_bias;
    const float *token_emb, *pos_emb, *lnf_g, *lnf_b, *proj_w, *proj_b;
    const mme_vit_layer* layer;
};
TextW text_w(const mme_clip_text_weights& w) {
    return TextW{TEXT_CLIP, w.hidden, w.layers, w.heads, w.mlp, w.vocab, TXT_T, w.proj_dim, w.act, w.eos_token_id, w.ln_eps, false, 0.f, 0.f,
                 w.token_emb, w.pos_emb, w.lnf_g, w.lnf_b, w.proj_w, nullptr, w.layer};
}
TextW text_w(const mme_siglip_text_weights& w) {
    return TextW{TEXT_SIGLIP, w.hidden, w.layers, w.heads, w.mlp, w.vocab, TXT_T64, w.projection_size, 2 /* tanh-GELU */, w.pad_token_id, w.ln_eps,
                 w.has_logits != 0, w.logit_scale, w.logit_bias, w.token_emb, w.pos_emb, w.lnf_g, w.lnf_b, w.head_w, w.head_b, w.layer};
}

int null_layer_tensor(mme_ctx* c, const char* who, const mme_vit_layer* layer, int layers) {
    for (int l = 0; l < layers; ++l) {
        const mme_vit_layer& a = layer[l];
        const float* all[] = {a.ln1_g, a.ln1_b, a.q_w, a.q_b, a.k_w, a.k_b, a.v_w, a.v_b, a.o_w, a.o_b, a.ln2_g, a.ln2_b, a.fc1_w, a.fc1_b, a.fc2_w, a.fc2_b};
        for (const float* p : all)
            if (!p) return fail(c, MME_E_ARG, "%s: layer %d has a null tensor pointer", who, l);
    }
    return MME_OK;
}

// the SigLIP text loaders' supported set (include/mme.h); as validate_text_weights below, nothing in the context changes
int validate_siglip_text_weights(mme_ctx* c, const mme_siglip_text_weights* w, const char* who) {
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    if (!text_width_built(w->hidden)) return fail(c, MME_E_ARG, "%s: hidden = %d; supported: 512, 768, 1024", who, w->hidden);
    if (w->heads * VIT_DH != w->hidden)
        return fail(c, MME_E_ARG, "%s: heads = %d at hidden = %d; supported: heads of %d, heads = hidden / %d = %d", who, w->heads, w->hidden, VIT_DH, VIT_DH,
                    w->hidden / VIT_DH);
    if (w->max_positions != TXT_T64) return fail(c, MME_E_ARG, "%s: max_positions = %d; supported: %d", who, w->max_positions, TXT_T64);
    if (w->mlp < 64 || (w->mlp % 64) != 0 || w->mlp > VIT_MAX_F)
        return fail(c, MME_E_ARG, "%s: mlp = %d; supported: multiples of 64 up to %d", who, w->mlp, VIT_MAX_F);
    if (w->layers < 1 || w->layers > VIT_MAX_L) return fail(c, MME_E_ARG, "%s: layers = %d; supported: 1..%d", who, w->layers, VIT_MAX_L);
    if (w->vocab < 3 || w->vocab > TXT_MAX_VOCAB_SIGLIP) return fail(c, MME_E_ARG, "%s: vocab = %d; supported: 3..%d", who, w->vocab, TXT_MAX_VOCAB_SIGLIP);
    if (w->projection_size < 64 || (w->projection_size % 64) != 0 || w->projection_size > 1024)
        return fail(c, MME_E_ARG, "%s: projection_size = %d; supported: a multiple of 64 up to 1024", who, w->projection_size);
    if (w->pad_token_id < 0 || w->pad_token_id >= w->vocab)
        return fail(c, MME_E_ARG, "%s: pad_token_id = %d; supported: 0..vocab-1 = 0..%d", who, w->pad_token_id, w->vocab - 1);
    if (!w->token_emb || !w->pos_emb || !w->lnf_g || !w->lnf_b || !w->head_w || !w->head_b || !w->layer)
        return fail(c, MME_E_ARG, "%s: null tensor pointer", who);
    return null_layer_tensor(c, who, w->layer, w->layers);
}

// every refusal names the field, the value found and what is supported; touches nothing in the context but its error text
int validate_text_weights(mme_ctx* c, const mme_clip_text_weights* w) {
    const char* who = "mme_load_clip_text";
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    if (!text_width_built(w->hidden)) return fail(c, MME_E_ARG, "%s: hidden = %d; supported: 512, 768, 1024", who, w->hidden);
    if (w->heads * VIT_DH != w->hidden)
        return fail(c, MME_E_ARG, "%s: heads = %d at hidden = %d; supported: heads of %d, heads = hidden / %d = %d", who, w->heads, w->hidden, VIT_DH, VIT_DH,
                    w->hidden / VIT_DH);
    if (w->max_positions != TXT_T) return fail(c, MME_E_ARG, "%s: max_positions = %d; supported: %d", who, w->max_positions, TXT_T);
    if (w->mlp < 64 || (w->mlp % 64) != 0 || w->mlp > VIT_MAX_F)
        return fail(c, MME_E_ARG, "%s: mlp = %d; supported: multiples of 64 up to %d", who, w->mlp, VIT_MAX_F);
    if (w->layers < 1 || w->layers > VIT_MAX_L) return fail(c, MME_E_ARG, "%s: layers = %d; supported: 1..%d", who, w->layers, VIT_MAX_L);
    if (w->vocab < 3 || w->vocab > TXT_MAX_VOCAB) return fail(c, MME_E_ARG, "%s: vocab = %d; supported: 3..%d", who, w->vocab, TXT_MAX_VOCAB);
    if (w->act != 0 && w->act != 1) return fail(c, MME_E_ARG, "%s: act = %d; supported: 0 (erf-GELU), 1 (QuickGELU)", who, w->act);
    if (w->proj_dim != 0 && (w->proj_dim < 64 || (w->proj_dim % 64) != 0 || w->proj_dim > 1024))
        return fail(c, MME_E_ARG, "%s: proj_dim = %d; supported: 0 (no projection) or a multiple of 64 up to 1024", who, w->proj_dim);
    if (w->eos_token_id < 0 || w->eos_token_id >= w->vocab)
        return fail(c, MME_E_ARG, "%s: eos_token_id = %d; supported: 0..vocab-1 = 0..%d", who, w->eos_token_id, w->vocab - 1);
    if ((w->proj_dim != 0) != (w->proj_w != nullptr))
        return fail(c, MME_E_ARG, "%s: proj_dim = %d with proj_w %s; supported: both set, or proj_dim = 0 with proj_w NULL", who, w->proj_dim,
                    w->proj_w ? "set" : "NULL");
    if (!w->token_emb || !w->pos_emb || !w->lnf_g || !w->lnf_b || !w->layer) return fail(c, MME_E_ARG, "%s: null tensor pointer", who);
    return null_layer_tensor(c, who, w->layer, w->layers);
}

// every tensor of the checkpoint with its element count (the order of the staged bytes)
template <class Fn>
void each_text_tensor(TextW& w, std::vector<mme_vit_layer>& layer, Fn&& f) {
    const size_t D = (size_t)w.hidden, F = (size_t)w.mlp;
    f(w.token_emb, (size_t)w.vocab * D);
    f(w.pos_emb, (size_t)w.tokens * D);
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
    if (w.proj_w) f(w.proj_w, (size_t)w.proj_dim * D);
    if (w.proj_b) f(w.proj_b, (size_t)w.proj_dim);
}

// The prepared buffers of the text tower, in the order mme_weights_fingerprint reports them: tok, pos, lnf_g, lnf_b, then
// 10 per layer, then proj_w and, for a head with bias (SigLIP), proj_b (include/mme.h).  Only the folded forms exist: there is
// no LayerNorm-kernel mode for text.
template <class P>
int prepare_text(mme_ctx* c, P& p, const TextW& w) {
    TextDev* t = c->text;
    int r;
    const size_t D = (size_t)w.hidden, F = (size_t)w.mlp;
    const size_t rD[3] = {D, D, D}, rF[1] = {F}, rV[1] = {(size_t)w.vocab};
    auto plain = [&](const float* src, size_t n, float** dst) { return p.table(src, n, 1.f, false, dst); };
    auto plain_bf16 = [&](const float* src, const size_t* rows, size_t cols, bf16_t** dst) {
        const void* s[1] = {src};
        return p.bf16(s, rows, 1, cols, 1.f, false, dst);
    };
    if ((r = plain_bf16(w.token_emb, rV, D, &t->tok))) return r;
    if ((r = plain(w.pos_emb, (size_t)w.tokens * D, &t->pos))) return r;
    if ((r = plain(w.lnf_g, D, &t->lnf_g))) return r;
    if ((r = plain(w.lnf_b, D, &t->lnf_b))) return r;
    const float sc = 0.125f * 1.44269504088896341f;  // dh^-0.5 * log2(e), folded into the query rows (weight_load.hip, prepare_vit)
    for (int l = 0; l < w.layers; ++l) {
        const mme_vit_layer& a = w.layer[l];
        BlockW& L = t->layer[l];
        const WpFoldSrc fq[3] = {{a.q_w, a.q_b, sc, 1}, {a.k_w, a.k_b, 1.f, 0}, {a.v_w, a.v_b, 1.f, 0}};
        if ((r = p.folded(fq, rD, 3, D, a.ln1_g, a.ln1_b, &L.qkv_wf, &L.qkv_cs, &L.qkv_bf))) return r;
        if ((r = plain_bf16(a.o_w, rD, D, &L.o_w))) return r;
        if ((r = plain(a.o_b, D, &L.o_b))) return r;
        const WpFoldSrc f1[1] = {{a.fc1_w, a.fc1_b, 1.f, 0}};
        if ((r = p.folded(f1, rF, 1, D, a.ln2_g, a.ln2_b, &L.fc1_wf, &L.fc1_cs, &L.fc1_bf))) return r;
        if ((r = plain_bf16(a.fc2_w, rD, F, &L.fc2_w))) return r;
        if ((r = plain(a.fc2_b, D, &L.fc2_b))) return r;
    }
    if (w.proj_w) {
        const size_t rP[1] = {(size_t)w.proj_dim};
        if ((r = plain_bf16(w.proj_w, rP, D, &t->proj_w))) return r;
    }
    if (w.proj_b && (r = plain(w.proj_b, (size_t)w.proj_dim, &t->proj_b))) return r;
    return MME_OK;
}

// A text load replaces the context's text tower and nothing else: it frees exactly the previous text buffers (after the
// device has drained), leaves the tower unloaded while it prepares, and marks what it allocated as the new range.
template <class P>
int load_text(mme_ctx* c, const TextW* w, P p, const char* who) {
    int r;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = text_dev(c, who))) return r;
    TextDev* t = c->text;
    t->loaded = false;
    if (c->text_alloc_hi > c->text_alloc_lo) HIP_TRY(c, hipDeviceSynchronize());  // a pass in flight still reads them
    release_alloc_range(c, c->text_alloc_lo, c->text_alloc_hi);
    t->hidden = w->hidden; t->layers = w->layers; t->heads = w->heads; t->mlp = w->mlp; t->vocab = w->vocab;
    t->proj_dim = w->proj_dim; t->act = w->act; t->eos = w->eos; t->eps = w->ln_eps;
    t->kind = w->kind; t->tokens = w->tokens; t->causal = w->kind == TEXT_CLIP; t->pool_last = w->kind == TEXT_SIGLIP; t->pad = w->eos;
    t->has_logits = w->has_logits; t->logit_scale = w->logit_scale; t->logit_bias = w->logit_bias;
    t->tok = nullptr; t->pos = t->lnf_g = t->lnf_b = nullptr; t->proj_w = nullptr; t->proj_b = nullptr;
    t->layer.assign((size_t)w->layers, BlockW{});
    std::vector<mme_vit_layer> layer(w->layer, w->layer + w->layers);
    TextW v = *w;
    v.layer = layer.data();
    r = p.stage([&](auto& put) { each_text_tensor(v, layer, put); });
    if (r == MME_OK) r = prepare_text(c, p, v);
    r = p.finish(r);
    c->text_alloc_hi = c->allocs.size();
    t->loaded = r == MME_OK;
    return r;
}

// host side of the pass's input: every id inside the table, and the EOS position of every sequence by transformers' rule
// (CLIPTextTransformer.forward): eos_token_id == 2 -> argmax of the ids (first of equals), else the first position that
// holds eos_token_id.  transformers pools position 0 when there is none (argmax of an all-zero mask); here that is an error.
int scan_ids(mme_ctx* c, const char* who, const int32_t* ids, int n, int vocab, int eos, std::vector<int32_t>& pos) {
    pos.resize((size_t)n);
    for (int b = 0; b < n; ++b) {
        const int32_t* row = ids + (size_t)b * TXT_T;
        int best = 0, found = -1;
        for (int t = 0; t < TXT_T; ++t) {
            if (row[t] < 0 || row[t] >= vocab)
                return fail(c, MME_E_ARG, "%s: sequence %d, position %d: id = %d; supported: 0..vocab-1 = 0..%d", who, b, t, row[t], vocab - 1);
            if (row[t] > row[best]) best = t;
            if (found < 0 && row[t] == eos) found = t;
        }
        if (eos == 2) found = best;
        if (found < 0) return fail(c, MME_E_ARG, "%s: sequence %d holds no eos_token_id = %d: there is no row to pool", who, b, eos);
        pos[(size_t)b] = found;
    }
    return MME_OK;
}

// the same check where the last position is pooled (SigLIP): ids against the vocabulary only, there is no EOS to find
int check_ids(mme_ctx* c, const char* who, const int32_t* ids, int n, int tokens, int vocab, std::vector<int32_t>& pos) {
    for (int b = 0; b < n; ++b)
        for (int t = 0; t < tokens; ++t) {
            const int32_t id = ids[(size_t)b * tokens + t];
            if (id < 0 || id >= vocab)
                return fail(c, MME_E_ARG, "%s: sequence %d, position %d: id = %d; supported: 0..vocab-1 = 0..%d", who, b, t, id, vocab - 1);
        }
    pos.assign((size_t)n, tokens - 1);
    return MME_OK;
}

// One chunk of either tower.  eos_dev holds the position to pool of every sequence: the EOS position (CLIP) or tokens - 1.
int text_chunk(mme_ctx* c, TextDev* t, const int32_t* ids_dev, const int32_t* eos_dev, int n, float* emb_f32, bf16_t* emb_bf16, hipStream_t s) {
    const int T = t->tokens;
    const int M = n * T, D = t->hidden, NL = t->layers;
    EncoderPass P{c, s, D, t->mlp, t->eps, t->act, t->x.p, t->qkv.p, t->att.p, t->hmlp.p, (float*)t->stats.p};
    P.planes = false;    // ln_mode is not consulted: the text tower runs mode 1, one statistics pass over x per LayerNorm,
    P.lnpart = nullptr;  // and its residual GEMMs are handed no planes
    P.zigzag = 0;        // every kernel walks the rows forwards
    int r;
    {
        Timed tm(c, s, KC_PRE);
        HIP_TRY(c, launch_text_token_rows(t->tok, t->pos, ids_dev, t->x.p, n, D, s, T));
    }
    if ((r = P.stats_from_x(t->x.p, 0, M))) return r;
    for (int l = 0; l < NL; ++l) {
        if ((r = P.qkv_ln(t->layer[l], M, 3 * D))) return r;
        {
            Timed tm(c, s, KC_ATTN);
            HIP_TRY(c, launch_attention_exact(t->qkv.p, t->att.p, n, T, t->causal, t->heads, s));
        }
        // no statistics after the last block: final_layer_norm touches the pooled rows only
        if ((r = P.after_attention(t->layer[l], M, t->att.p, t->x.p, l + 1 < NL))) return r;
    }
    const int E = t->proj_dim;
    {
        Timed tm(c, s, KC_POOL);
        HIP_TRY(c, launch_text_eos_pool_ln(t->x.p, t->lnf_g, t->lnf_b, eos_dev, n, D, t->eps, E ? t->pooled.p : nullptr, E ? nullptr : (float*)t->projf.p, s, T));
    }
    if (E) {
        GemmArgs g{};
        g.A = t->pooled.p; g.W = t->proj_w; g.M = n; g.N = E; g.K = D;
        g.outf = (float*)t->projf.p; g.ldf = E;
        if ((r = P.gemm(EPI_F32, g))) return r;
    }
    Timed tm(c, s, KC_POOL);
    if (t->proj_b) HIP_TRY(c, launch_bias_l2_rows((const float*)t->projf.p, t->proj_b, n, E, emb_f32, emb_bf16, s));
    else HIP_TRY(c, launch_l2_rows((const float*)t->projf.p, n, E ? E : D, emb_f32, emb_bf16, s));
    return MME_OK;
}

}  // namespace

extern "C" {

int mme_load_clip_text(mme_ctx* c, const mme_clip_text_weights* w) {
    int r;
    if ((r = validate_text_weights(c, w))) return r;
    const TextW v = text_w(*w);
    return load_text(c, &v, HostPrep{c}, "mme_load_clip_text");
}

int mme_load_clip_text_as(mme_ctx* c, const mme_clip_text_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_text_weights(c, w))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_clip_text_as"))) return r;
    const TextW v = text_w(*w);
    return load_text(c, &v, DevPrep(c, dtype, stream, "mme_load_clip_text_as"), "mme_load_clip_text_as");
}

int mme_load_siglip_text(mme_ctx* c, const mme_siglip_text_weights* w) {
    int r;
    if ((r = validate_siglip_text_weights(c, w, "mme_load_siglip_text"))) return r;
    const TextW v = text_w(*w);
    return load_text(c, &v, HostPrep{c}, "mme_load_siglip_text");
}

int mme_load_siglip_text_as(mme_ctx* c, const mme_siglip_text_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_siglip_text_weights(c, w, "mme_load_siglip_text_as"))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_siglip_text_as"))) return r;
    const TextW v = text_w(*w);
    return load_text(c, &v, DevPrep(c, dtype, stream, "mme_load_siglip_text_as"), "mme_load_siglip_text_as");
}

int mme_text_geometry(mme_ctx* c, int32_t out[4]) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_text_geometry: null argument");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    const TextDev* t = c->text;
    if (!t || !t->loaded) return MME_OK;
    out[0] = t->kind; out[1] = t->tokens; out[2] = t->proj_dim; out[3] = t->kind == TEXT_SIGLIP ? t->pad : t->eos;
    return MME_OK;
}

int mme_siglip_scores(mme_ctx* c, const float* cos_f32, int64_t m, int64_t N, float* out_f32, void* stream) {
    if (!c) return MME_E_ARG;
    const TextDev* t = c->text;
    if (!t || !t->loaded || t->kind != TEXT_SIGLIP || !t->has_logits)
        return fail(c, MME_E_STATE, "mme_siglip_scores: needs a SigLIP text tower loaded with logit_scale and logit_bias (a whole SiglipModel)");
    if (m < 0 || N < 0 || (N > 0 && m > INT64_MAX / 8 / N)) return fail(c, MME_E_ARG, "mme_siglip_scores: m = %lld, N = %lld", (long long)m, (long long)N);
    if (m * N == 0) return MME_OK;
    if (!cos_f32 || !out_f32 || ((uintptr_t)cos_f32 & 3) || ((uintptr_t)out_f32 & 3)) return fail(c, MME_E_ARG, "mme_siglip_scores: cos_f32 and out_f32 non-null f32 buffers");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    Timed tm(c, s, KC_COS);
    HIP_TRY(c, launch_siglip_scores(cos_f32, out_f32, m * N, expf(t->logit_scale), t->logit_bias, s));
    return MME_OK;
}

int mme_text_info(mme_ctx* c, int32_t out[9]) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_text_info: null argument");
    for (int i = 0; i < 9; ++i) out[i] = 0;
    const TextDev* t = c->text;
    if (!t || !t->loaded) return MME_OK;
    const int32_t v[9] = {1, t->hidden, t->layers, t->heads, t->mlp, t->vocab, t->proj_dim, t->act, t->eos};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return MME_OK;
}

int mme_text_forward(mme_ctx* c, const int32_t* ids_host, int n, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    TextDev* t = c->text;
    if (!t || !t->loaded) return fail(c, MME_E_STATE, "mme_text_forward: call mme_load_clip_text first");
    if (n < 0 || (n > 0 && !ids_host)) return fail(c, MME_E_ARG, "mme_text_forward: null ids or n<0");
    if (n == 0) return MME_OK;
    std::vector<int32_t> eos_pos;
    int r;
    const size_t T = (size_t)t->tokens;
    if (t->pool_last) r = check_ids(c, "mme_text_forward", ids_host, n, t->tokens, t->vocab, eos_pos);
    else r = scan_ids(c, "mme_text_forward", ids_host, n, t->vocab, t->eos, eos_pos);
    if (r) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    const int chunk = n < MME_TEXT_CHUNK ? n : MME_TEXT_CHUNK;
    const size_t rows = (size_t)chunk * T, D = (size_t)t->hidden, F = (size_t)t->mlp, E = (size_t)text_embed_dim(t);
    if ((r = ensure(c, t->x, rows * D * 2))) return r;
    if ((r = ensure(c, t->qkv, rows * 3 * D * 2))) return r;
    if ((r = ensure(c, t->att, rows * D * 2))) return r;
    if ((r = ensure(c, t->hmlp, rows * F * 2))) return r;
    if ((r = ensure(c, t->stats, rows * 2 * sizeof(float)))) return r;
    if ((r = ensure(c, t->pooled, (size_t)chunk * D * 2))) return r;
    if ((r = ensure(c, t->projf, (size_t)chunk * (E > D ? E : D) * sizeof(float)))) return r;
    if ((r = ensure(c, t->ids, (size_t)n * T * sizeof(int32_t)))) return r;
    if ((r = ensure(c, t->eos_pos, (size_t)n * sizeof(int32_t)))) return r;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(c, hipMemcpyAsync(t->ids.p, ids_host, (size_t)n * T * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(t->eos_pos.p, eos_pos.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // eos_pos is a local; the caller's ids may be released on return
    for (int s0 = 0; s0 < n; s0 += MME_TEXT_CHUNK) {
        const int m = n - s0 < MME_TEXT_CHUNK ? n - s0 : MME_TEXT_CHUNK;
        r = text_chunk(c, t, (const int32_t*)t->ids.p + (size_t)s0 * T, (const int32_t*)t->eos_pos.p + s0, m,
                       emb_f32 ? emb_f32 + (size_t)s0 * E : nullptr, emb_bf16 ? (bf16_t*)emb_bf16 + (size_t)s0 * E : nullptr, s);
        if (r) return r;
    }
    return MME_OK;
}

}  // extern "C"

namespace {

// Ops 0..2 of mme_text_apply and mme_siglip_text_apply -- token rows, exact attention, the pooled LayerNorm -- one launch
// each at the text layout L.  What differs: the vocabulary cap, whether attention takes only_block, and the pooled
// positions, the caller's (eos_pos_host, CLIP) or tokens - 1 for every sequence (null: SigLIP).  A is either hook's args struct.
template <class A>
int text_steps_apply(mme_ctx* c, const char* who, const TokenLayout& L, int op, const A* a, int vocab_cap, int only_block, const int32_t* eos_pos_host,
                     bool pool_last, void* stream) {
    const HookCheck h{c, who, op};
    const char* bad = nullptr;
    const int n = a->n, T = L.tokens;
    if (int r = h.crops(n)) return r;
    if (op != 1 && !text_width_built(a->d)) return fail(c, MME_E_ARG, "%s: op %d is built for d == 512, d == 768 and d == 1024 (d = %d)", who, op, a->d);
    if (op == 0) {
        if (!vec16(a->tok) || !vec16(a->pos) || !vec16(a->x) || !a->ids_host) bad = "tok, pos, x non-null and 16-byte aligned, ids_host non-null";
        else if (a->vocab < 1 || a->vocab > vocab_cap) return fail(c, MME_E_ARG, "%s: op %d needs 1 <= vocab <= %d", who, op, vocab_cap);
    } else if (op == 1) {
        if (int r = h.heads(L, a->heads)) return r;
        if (!L.takes_block(only_block)) return fail(c, MME_E_ARG, "%s: op 1: only_block = %d outside -1..%d", who, only_block, L.blocks - 1);
        if (!vec16(a->qkv) || !vec16(a->out)) bad = "qkv, out non-null and 16-byte aligned";
    } else {
        if (!vec16(a->x) || !vec16(a->gamma) || !vec16(a->beta) || (!pool_last && !eos_pos_host))
            bad = pool_last ? "x, gamma, beta non-null and 16-byte aligned" : "x, gamma, beta non-null and 16-byte aligned, eos_pos_host non-null";
        else if (int r = h.out_pair(a->y, a->y_f32, "y", "y_f32")) return r;
    }
    if (bad) return h.needs(bad);
    if (op == 0)
        for (size_t i = 0; i < (size_t)n * T; ++i)
            if (a->ids_host[i] < 0 || a->ids_host[i] >= a->vocab)
                return fail(c, MME_E_ARG, "%s: op 0: ids_host[%zu] = %d outside 0..vocab-1 = 0..%d", who, i, a->ids_host[i], a->vocab - 1);
    if (op == 2 && !pool_last)
        for (int b = 0; b < n; ++b)
            if (eos_pos_host[b] < 0 || eos_pos_host[b] >= T)
                return fail(c, MME_E_ARG, "%s: op 2: eos_pos_host[%d] = %d outside 0..%d", who, b, eos_pos_host[b], T - 1);
    if (n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (op != 1) {  // the ids, or the position to pool of every sequence
        if ((r = text_dev(c, who))) return r;
        std::vector<int32_t> last;
        if (op == 2 && pool_last) last.assign((size_t)n, T - 1);
        const size_t bytes = (op == 0 ? (size_t)n * T : (size_t)n) * sizeof(int32_t);
        if ((r = ensure(c, c->text->apply_ints, bytes))) return r;
        HIP_TRY(c, hipMemcpyAsync(c->text->apply_ints.p, op == 0 ? a->ids_host : pool_last ? last.data() : eos_pos_host, bytes, hipMemcpyHostToDevice, s));
        if (pool_last) HIP_TRY(c, hipStreamSynchronize(s));  // `last` is a local
    }
    const int32_t* ints = op != 1 ? (const int32_t*)c->text->apply_ints.p : nullptr;
    switch (op) {
        case 0: HIP_TRY(c, launch_text_token_rows(a->tok, a->pos, ints, a->x, n, a->d, s, T)); break;
        case 1: HIP_TRY(c, launch_attention_exact(a->qkv, a->out, n, T, L.causal, a->heads, s, only_block)); break;
        default: HIP_TRY(c, launch_text_eos_pool_ln(a->x, a->gamma, a->beta, ints, n, a->d, a->eps, a->y, a->y_f32, s, T)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // namespace

extern "C" {

// the kernels the text tower adds, one launch each (tests/test_gpu_clip_text.py)
int mme_text_apply(mme_ctx* c, int op, const mme_text_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_text_apply", a, op, 2)) return r;
    return text_steps_apply(c, "mme_text_apply", *find_layout(TXT_T), op, a, TXT_MAX_VOCAB, -1, a->eos_pos_host, false, stream);
}

// the kernels the SigLIP text tower adds, one launch each (tests/test_gpu_siglip_text.py)
int mme_siglip_text_apply(mme_ctx* c, int op, const mme_siglip_text_apply_args* a, void* stream) {
    const char* who = "mme_siglip_text_apply";
    if (int r = hook_args(c, who, a, op, 4)) return r;
    if (op <= 2) return text_steps_apply(c, who, *find_layout(TXT_T64), op, a, TXT_MAX_VOCAB_SIGLIP, a->only_block, nullptr, true, stream);
    const HookCheck h{c, who, op};
    const char* bad = nullptr;
    if (int r = h.crops(a->n)) return r;
    if (op == 3) {
        if (a->p < 64 || (a->p % 64) != 0 || a->p > 1024) return fail(c, MME_E_ARG, "%s: op 3: p = %d; supported: a multiple of 64 up to 1024", who, a->p);
        if (!vec16(a->acc) || !vec16(a->bias)) bad = "acc, bias non-null and 16-byte aligned";
        else if (int r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16")) return r;
    } else {
        if (a->count < 0) return fail(c, MME_E_ARG, "%s: op 4: count = %lld", who, (long long)a->count);
        if (!a->cos || !a->scores || ((uintptr_t)a->cos & 3) || ((uintptr_t)a->scores & 3)) bad = "cos, scores non-null and 4-byte aligned";
    }
    if (bad) return fail(c, MME_E_ARG, "%s: op %d needs %s", who, op, bad);
    if (op == 4 ? a->count == 0 : a->n == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (op == 3) HIP_TRY(c, launch_bias_l2_rows(a->acc, a->bias, a->n, a->p, a->emb_f32, a->emb_bf16, s));
    else HIP_TRY(c, launch_siglip_scores(a->cos, a->scores, a->count, expf(a->logit_scale), a->logit_bias, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // extern "C"
