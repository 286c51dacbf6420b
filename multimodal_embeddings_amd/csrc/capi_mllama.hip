// C ABI of the Mllama language tower (include/mme.h, "Mllama language tower with cross-attention"):
// transformers' multi_modal_projector + MllamaTextModel on the MFMA GEMM of the image path (launch_gemm, bf16, f32
// accumulation) with the tower's own kernels (mllama_lm.hip).  The tower lives beside the context's other towers: its record
// and workspace are here, its prepared buffers in c->allocs[mllama_alloc_lo, mllama_alloc_hi).
//
// One pass over a chunk of n sequences of S tokens (M = n S rows), V = n * tiles * tokens vision rows:
//   x = embed_tokens[ids]                                             gather
//   vis = states . proj_w^T + proj_b                                  GEMM [V, hidden]          (image path, once per chunk)
//   self layer:  h = rmsnorm(x, ln1); qkv = h . (q | k | v)^T; RoPE on Q | K; att = causal GQA attention;
//                x += att . o^T; h = rmsnorm(x, ln2); gu = h . (gate | up)^T; a = silu(g) * u; x += a . down^T
//   cross layer (skipped without vision rows):
//                h = rmsnorm(x, ln1); q = headnorm(h . q^T, q_norm); kv = vis . (k | v)^T, headnorm on K with k_norm;
//                att = masked attention over the V / n keys of the image; x += att . (tanh(attn_gate) o)^T;
//                h = rmsnorm(x, ln2); a = silu(g) * u with the rows that attend no tile zeroed; x += a . (tanh(mlp_gate) down)^T
//   emb = l2(w_norm * rmsnorm(x[len - 1]))
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "ctx.h"
#include "mllama_lm.h"

namespace {
constexpr int ML_MAX_LAYERS = 64, ML_MAX_HEADS = 64, ML_MAX_I = 16384, ML_MAX_ROWS = 1 << 18, ML_MAX_VISION = 8192, ML_MAX_TILES = 4, ML_MAX_TOKENS = 1601;
constexpr int ML_CHUNK = 64;

struct MllamaLayerDev {
    bool cross = false;
    float *ln1 = nullptr, *ln2 = nullptr, *qn = nullptr, *kn = nullptr;
    bf16_t *qkv_w = nullptr;  // self: q | k | v; cross: q
    bf16_t *kv_w = nullptr;   // cross: k | v
    bf16_t *o_w = nullptr, *gu_w = nullptr, *down_w = nullptr;
};
}  // namespace

struct MllamaDev {
    bool loaded = false;
    int hidden = 0, heads = 0, kv_heads = 0, inter = 0, layers = 0, ncross = 0, vocab = 0, vision_dim = 0, image_token = 0, rope_type = 0;
    float eps = 1e-5f;
    bf16_t *embed = nullptr, *proj_w = nullptr;
    float *norm = nullptr, *proj_b = nullptr, *zeros = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    std::vector<MllamaLayerDev> layer;
    std::vector<float> h_cos, h_sin;  // the rotary tables while they are uploaded
    // workspace of the pass (grown, never shrunk) and the staging of a call's integers
    DevBuf x, h, qkv, att, gu, act, vis, kv, cross_ws, ids, len, xm, rowzero, states, apply_ints;
};

void mllama_free(mme_ctx* c) {
    if (!c->mllama) return;
    MllamaDev* t = c->mllama;
    DevBuf* bufs[] = {&t->x, &t->h, &t->qkv, &t->att, &t->gu, &t->act, &t->vis, &t->kv, &t->cross_ws, &t->ids, &t->len, &t->xm, &t->rowzero, &t->states, &t->apply_ints};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    delete t;
    c->mllama = nullptr;
}

namespace {

int mllama_dev(mme_ctx* c, const char* who) {
    if (c->mllama) return MME_OK;
    c->mllama = new (std::nothrow) MllamaDev();
    if (!c->mllama) return fail(c, MME_E_NOMEM, "%s: out of host memory", who);
    return MME_OK;
}

bool group_built(int heads, int kv_heads) {
    if (kv_heads < 1 || heads % kv_heads) return false;
    const int g = heads / kv_heads;
    return g == 1 || g == 2 || g == 4 || g == 8;
}

// every refusal names the field, the value found and what is supported; touches nothing in the context but its error text
int validate_mllama(mme_ctx* c, const mme_mllama_lm_weights* w, const char* who) {
    if (!c || !w) return fail(c, MME_E_ARG, "%s: null argument", who);
    if (w->heads < 1 || w->heads > ML_MAX_HEADS) return fail(c, MME_E_ARG, "%s: heads = %d; supported: 1..%d", who, w->heads, ML_MAX_HEADS);
    if (w->hidden != w->heads * MLLAMA_DH)
        return fail(c, MME_E_ARG, "%s: hidden = %d at heads = %d; supported: heads of %d, hidden = heads * %d = %d", who, w->hidden, w->heads, MLLAMA_DH,
                    MLLAMA_DH, w->heads * MLLAMA_DH);
    if (!group_built(w->heads, w->kv_heads))
        return fail(c, MME_E_ARG, "%s: kv_heads = %d at heads = %d; supported: heads / kv_heads in {1, 2, 4, 8}", who, w->kv_heads, w->heads);
    if (w->intermediate < 64 || (w->intermediate % 64) != 0 || w->intermediate > ML_MAX_I)
        return fail(c, MME_E_ARG, "%s: intermediate = %d; supported: multiples of 64 up to %d", who, w->intermediate, ML_MAX_I);
    if (w->layers < 1 || w->layers > ML_MAX_LAYERS) return fail(c, MME_E_ARG, "%s: layers = %d; supported: 1..%d", who, w->layers, ML_MAX_LAYERS);
    if (w->vocab < 1 || w->vocab + 8 > ML_MAX_ROWS) return fail(c, MME_E_ARG, "%s: vocab = %d; supported: 1..%d (vocab + 8 rows <= 2^18)", who, w->vocab, ML_MAX_ROWS - 8);
    if (w->vision_dim < 64 || (w->vision_dim % 64) != 0 || w->vision_dim > ML_MAX_VISION)
        return fail(c, MME_E_ARG, "%s: vision_dim = %d; supported: multiples of 64 up to %d", who, w->vision_dim, ML_MAX_VISION);
    if (w->image_token_id < 0 || w->image_token_id >= w->vocab + 8)
        return fail(c, MME_E_ARG, "%s: image_token_id = %d; supported: 0..vocab + 7 = 0..%d", who, w->image_token_id, w->vocab + 7);
    if (w->hidden_act != 0) return fail(c, MME_E_ARG, "%s: hidden_act = %d; supported: 0 (silu)", who, w->hidden_act);
    if (w->rope_type != 0 && w->rope_type != 1) return fail(c, MME_E_ARG, "%s: rope_type = %d; supported: 0 (default), 1 (llama3)", who, w->rope_type);
    if (!(w->rope_theta > 0.f)) return fail(c, MME_E_ARG, "%s: rope_theta = %g; supported: > 0", who, (double)w->rope_theta);
    if (w->rope_type == 1 && (!(w->rope_factor > 0.f) || w->rope_original_max < 1 || !(w->rope_high_freq_factor > w->rope_low_freq_factor) ||
                              !(w->rope_low_freq_factor > 0.f)))
        return fail(c, MME_E_ARG, "%s: llama3 rope factor = %g, low_freq_factor = %g, high_freq_factor = %g, original_max = %d; supported: factor > 0, 0 < low < high, original_max >= 1",
                    who, (double)w->rope_factor, (double)w->rope_low_freq_factor, (double)w->rope_high_freq_factor, w->rope_original_max);
    if (!(w->rms_eps > 0.f)) return fail(c, MME_E_ARG, "%s: rms_eps = %g; supported: > 0", who, (double)w->rms_eps);
    if (!w->embed_tokens || !w->norm || !w->proj_w || !w->proj_b || !w->layer) return fail(c, MME_E_ARG, "%s: null tensor pointer", who);
    for (int l = 0; l < w->layers; ++l) {
        const mme_mllama_lm_layer& a = w->layer[l];
        const float* all[] = {a.ln1, a.ln2, a.q_w, a.k_w, a.v_w, a.o_w, a.gate_w, a.up_w, a.down_w};
        for (const float* p : all)
            if (!p) return fail(c, MME_E_ARG, "%s: layer %d has a null tensor pointer", who, l);
        if (a.cross != 0 && a.cross != 1) return fail(c, MME_E_ARG, "%s: layer %d: cross = %d; supported: 0, 1", who, l, a.cross);
        if (a.cross && (!a.q_norm || !a.k_norm)) return fail(c, MME_E_ARG, "%s: cross layer %d has a null q_norm / k_norm", who, l);
    }
    return MME_OK;
}

// every tensor of the checkpoint with its element count (the order of the staged bytes)
template <class Fn>
void each_mllama_tensor(mme_mllama_lm_weights& w, std::vector<mme_mllama_lm_layer>& layer, Fn&& f) {
    const size_t D = (size_t)w.hidden, KV = (size_t)w.kv_heads * MLLAMA_DH, I = (size_t)w.intermediate;
    f(w.embed_tokens, (size_t)(w.vocab + 8) * D);
    f(w.norm, D);
    f(w.proj_w, D * (size_t)w.vision_dim);
    f(w.proj_b, D);
    for (mme_mllama_lm_layer& a : layer) {
        f(a.ln1, D); f(a.ln2, D);
        f(a.q_w, D * D); f(a.k_w, KV * D); f(a.v_w, KV * D); f(a.o_w, D * D);
        if (a.cross) { f(a.q_norm, (size_t)MLLAMA_DH); f(a.k_norm, (size_t)MLLAMA_DH); }
        f(a.gate_w, I * D); f(a.up_w, I * D); f(a.down_w, D * I);
    }
}

// transformers' rotary tables at positions 0..127 (modeling_rope_utils.py: _compute_default_rope_parameters,
// _compute_llama3_parameters; attention_scaling 1): inv_freq in f32 arithmetic as torch forms it, the angle pos * inv_freq in
// f32, cos / sin of that angle rounded to f32
void rope_tables(const mme_mllama_lm_weights& w, std::vector<float>& cs, std::vector<float>& sn) {
    const int half = MLLAMA_DH / 2;
    cs.assign((size_t)MLLAMA_MAX_S * half, 0.f);
    sn.assign((size_t)MLLAMA_MAX_S * half, 0.f);
    const float pi2 = 2.0f * 3.14159265358979323846f;
    for (int i = 0; i < half; ++i) {
        const float e = (float)(2 * i) / (float)MLLAMA_DH;
        float inv = 1.0f / (float)std::pow((double)w.rope_theta, (double)e);
        if (w.rope_type == 1) {
            const float low_wl = (float)w.rope_original_max / w.rope_low_freq_factor, high_wl = (float)w.rope_original_max / w.rope_high_freq_factor;
            const float wl = pi2 / inv;
            const float inv_l = wl > low_wl ? inv / w.rope_factor : inv;
            const float smooth = ((float)w.rope_original_max / wl - w.rope_low_freq_factor) / (w.rope_high_freq_factor - w.rope_low_freq_factor);
            const float smoothed = (1.0f - smooth) * inv_l / w.rope_factor + smooth * inv_l;
            const bool medium = !(wl < high_wl) && !(wl > low_wl);
            inv = medium ? smoothed : inv_l;
        }
        for (int p = 0; p < MLLAMA_MAX_S; ++p) {
            const float ang = (float)p * inv;
            cs[(size_t)p * half + i] = (float)std::cos((double)ang);
            sn[(size_t)p * half + i] = (float)std::sin((double)ang);
        }
    }
}

hipStream_t prep_stream(HostPrep&) { return nullptr; }
hipStream_t prep_stream(DevPrep& p) { return p.s; }

template <class P>
int prepare_mllama(mme_ctx* c, P& p, const mme_mllama_lm_weights& w) {
    MllamaDev* t = c->mllama;
    int r;
    const size_t D = (size_t)w.hidden, KV = (size_t)w.kv_heads * MLLAMA_DH, I = (size_t)w.intermediate;
    auto plain = [&](const float* src, size_t n, float** dst) { return p.table(src, n, 1.f, false, dst); };
    auto mats = [&](std::initializer_list<const float*> srcs, std::initializer_list<size_t> rows, size_t cols, float scale, bf16_t** dst) {
        const void* s[3] = {nullptr, nullptr, nullptr};
        size_t rr[3] = {0, 0, 0};
        int k = 0;
        for (const float* q : srcs) s[k++] = q;
        k = 0;
        for (size_t q : rows) rr[k++] = q;
        return p.bf16(s, rr, k, cols, scale, scale != 1.0f, dst);
    };
    if ((r = mats({w.embed_tokens}, {(size_t)(w.vocab + 8)}, D, 1.f, &t->embed))) return r;
    if ((r = plain(w.norm, D, &t->norm))) return r;
    if ((r = mats({w.proj_w}, {D}, (size_t)w.vision_dim, 1.f, &t->proj_w))) return r;
    if ((r = plain(w.proj_b, D, &t->proj_b))) return r;
    const size_t nz = 2 * I > D + 2 * KV ? 2 * I : D + 2 * KV;
    if ((r = p.zeros(nz, &t->zeros))) return r;
    rope_tables(w, t->h_cos, t->h_sin);
    if ((r = p.zeros(t->h_cos.size(), &t->rope_cos))) return r;
    if ((r = p.zeros(t->h_sin.size(), &t->rope_sin))) return r;
    hipStream_t ps = prep_stream(p);
    HIP_TRY(c, hipMemcpyAsync(t->rope_cos, t->h_cos.data(), t->h_cos.size() * sizeof(float), hipMemcpyHostToDevice, ps));
    HIP_TRY(c, hipMemcpyAsync(t->rope_sin, t->h_sin.data(), t->h_sin.size() * sizeof(float), hipMemcpyHostToDevice, ps));
    for (int l = 0; l < w.layers; ++l) {
        const mme_mllama_lm_layer& a = w.layer[l];
        MllamaLayerDev& L = t->layer[l];
        L.cross = a.cross != 0;
        if ((r = plain(a.ln1, D, &L.ln1))) return r;
        if (!L.cross) {
            if ((r = mats({a.q_w, a.k_w, a.v_w}, {D, KV, KV}, D, 1.f, &L.qkv_w))) return r;
            if ((r = mats({a.o_w}, {D}, D, 1.f, &L.o_w))) return r;
        } else {
            // x + tanh(gate) * branch(x): the gate multiplies the branch's LAST linear map, in f32 before the rounding to bf16
            if ((r = mats({a.q_w}, {D}, D, 1.f, &L.qkv_w))) return r;
            if ((r = plain(a.q_norm, (size_t)MLLAMA_DH, &L.qn))) return r;
            if ((r = plain(a.k_norm, (size_t)MLLAMA_DH, &L.kn))) return r;
            if ((r = mats({a.k_w, a.v_w}, {KV, KV}, D, 1.f, &L.kv_w))) return r;
            const void* o_w = a.o_w;
            const size_t rD[1] = {D};
            if ((r = p.bf16(&o_w, rD, 1, D, std::tanh(a.attn_gate), true, &L.o_w))) return r;
        }
        if ((r = plain(a.ln2, D, &L.ln2))) return r;
        if ((r = mats({a.gate_w, a.up_w}, {I, I}, D, 1.f, &L.gu_w))) return r;
        if (!L.cross) {
            if ((r = mats({a.down_w}, {D}, I, 1.f, &L.down_w))) return r;
        } else {
            const void* d_w = a.down_w;
            const size_t rD[1] = {D};
            if ((r = p.bf16(&d_w, rD, 1, I, std::tanh(a.mlp_gate), true, &L.down_w))) return r;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(ps));  // the rotary tables have left the host vectors
    return MME_OK;
}

// A load replaces the context's language tower and nothing else (as load_text, capi_text.hip)
template <class P>
int load_mllama(mme_ctx* c, const mme_mllama_lm_weights* w, P p, const char* who) {
    int r;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = mllama_dev(c, who))) return r;
    MllamaDev* t = c->mllama;
    t->loaded = false;
    if (c->mllama_alloc_hi > c->mllama_alloc_lo) HIP_TRY(c, hipDeviceSynchronize());  // a pass in flight still reads them
    release_alloc_range(c, c->mllama_alloc_lo, c->mllama_alloc_hi);
    t->hidden = w->hidden; t->heads = w->heads; t->kv_heads = w->kv_heads; t->inter = w->intermediate; t->layers = w->layers;
    t->vocab = w->vocab; t->vision_dim = w->vision_dim; t->image_token = w->image_token_id; t->rope_type = w->rope_type; t->eps = w->rms_eps;
    t->layer.assign((size_t)w->layers, MllamaLayerDev{});
    t->ncross = 0;
    for (int l = 0; l < w->layers; ++l) t->ncross += w->layer[l].cross != 0;
    std::vector<mme_mllama_lm_layer> layer(w->layer, w->layer + w->layers);
    mme_mllama_lm_weights v = *w;
    v.layer = layer.data();
    r = p.stage([&](auto& put) { each_mllama_tensor(v, layer, put); });
    if (r == MME_OK) r = prepare_mllama(c, p, v);
    r = p.finish(r);
    c->mllama_alloc_hi = c->allocs.size();
    t->loaded = r == MME_OK;
    return r;
}

int ml_gemm(mme_ctx* c, hipStream_t s, int epi, const void* A, const bf16_t* W, int M, int N, int K, const float* bias, void* out, const void* res) {
    GemmArgs g{};
    g.A = A; g.W = W; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out = out; g.ldo = N; g.res = res;
    Timed tm(c, s, KC_GEMM);
    HIP_TRY(c, launch_gemm(epi, g, s, c->gemm_variant));
    return MME_OK;
}

// What a call's host arrays say, checked before anything is launched: ids inside the table, lengths 1..S, and with vision
// rows the mask of every row (the caller's bits, or the processor's rule) and the rows whose cross MLP term is zero.
int scan_sequences(mme_ctx* c, const char* who, const MllamaDev* t, const int32_t* ids, const int32_t* len, int n, int S, bool vision, int tiles,
                   const int32_t* num_tiles, const uint8_t* xmask, std::vector<uint8_t>& xm, std::vector<uint8_t>& rowzero) {
    const int rows_v = t->vocab + 8;
    if (vision) {
        xm.assign((size_t)n * S, 0);
        rowzero.assign((size_t)n * S, 0);
    }
    for (int b = 0; b < n; ++b) {
        if (len[b] < 1 || len[b] > S) return fail(c, MME_E_ARG, "%s: sequence %d: len = %d; supported: 1..S = 1..%d", who, b, len[b], S);
        int first = -1;
        for (int i = 0; i < S; ++i) {
            const int32_t id = ids[(size_t)b * S + i];
            if (id < 0 || id >= rows_v) return fail(c, MME_E_ARG, "%s: sequence %d, position %d: id = %d; supported: 0..vocab + 7 = 0..%d", who, b, i, id, rows_v - 1);
            if (first < 0 && id == t->image_token) first = i;
        }
        if (!vision) continue;
        if (first < 0) return fail(c, MME_E_ARG, "%s: sequence %d holds no image_token_id = %d, but vision rows were given", who, b, t->image_token);
        if (!xmask && (num_tiles[b] < 1 || num_tiles[b] > tiles))
            return fail(c, MME_E_ARG, "%s: image %d has %d tiles; supported: 1..tiles = 1..%d", who, b, num_tiles[b], tiles);
        for (int i = 0; i < S; ++i) {
            const int bits = xmask ? xmask[(size_t)b * S + i] : (i >= first ? (1 << num_tiles[b]) - 1 : 0);
            if (bits >= (1 << tiles)) return fail(c, MME_E_ARG, "%s: sequence %d, position %d: mask bits = 0x%x; supported: below 1 << tiles = 0x%x", who, b, i, bits, 1 << tiles);
            xm[(size_t)b * S + i] = (uint8_t)bits;
            rowzero[(size_t)b * S + i] = bits == 0;
        }
    }
    return MME_OK;
}

int ensure_lm_workspace(mme_ctx* c, MllamaDev* t, int cap, int S, bool vision, int Nk) {
    const size_t rows = (size_t)cap * S, D = (size_t)t->hidden, KV = (size_t)t->kv_heads * MLLAMA_DH, I = (size_t)t->inter;
    int r;
    if ((r = ensure(c, t->x, rows * D * 2))) return r;
    if ((r = ensure(c, t->h, rows * D * 2))) return r;
    if ((r = ensure(c, t->qkv, rows * (D + 2 * KV) * 2))) return r;
    if ((r = ensure(c, t->att, rows * D * 2))) return r;
    if ((r = ensure(c, t->gu, rows * 2 * I * 2))) return r;
    if ((r = ensure(c, t->act, rows * I * 2))) return r;
    if ((r = ensure(c, t->ids, rows * sizeof(int32_t)))) return r;
    if ((r = ensure(c, t->len, (size_t)cap * sizeof(int32_t)))) return r;
    if (vision && t->ncross) {
        const size_t V = (size_t)cap * Nk;
        if ((r = ensure(c, t->vis, V * D * 2))) return r;
        if ((r = ensure(c, t->kv, V * 2 * KV * 2))) return r;
        if ((r = ensure(c, t->cross_ws, mllama_cross_workspace_floats(cap, S, t->heads, Nk) * sizeof(float)))) return r;
        if ((r = ensure(c, t->xm, rows))) return r;
        if ((r = ensure(c, t->rowzero, rows))) return r;
    }
    return MME_OK;
}

// One chunk of m sequences; the chunk's ids / len / masks are on the device (t->ids, t->len, t->xm, t->rowzero).
// states: bf16 [m * Nk, vision_dim] or null (text only)
int lm_chunk(mme_ctx* c, MllamaDev* t, int m, int S, const void* states, int tiles, int tokens, float* emb_f32, bf16_t* emb_bf16, hipStream_t s) {
    const int M = m * S, D = t->hidden, H = t->heads, KVH = t->kv_heads, KV = KVH * MLLAMA_DH, I = t->inter, Nk = tiles * tokens;
    const bool vision = states != nullptr && t->ncross > 0;
    int r;
    {
        Timed tm(c, s, KC_PRE);
        HIP_TRY(c, launch_mllama_gather(t->embed, (const int32_t*)t->ids.p, t->x.p, M, D, s));
    }
    if (vision && (r = ml_gemm(c, s, EPI_BIAS, states, t->proj_w, m * Nk, D, t->vision_dim, t->proj_b, t->vis.p, nullptr))) return r;
    for (int l = 0; l < t->layers; ++l) {
        const MllamaLayerDev& L = t->layer[l];
        if (L.cross && !vision) continue;  // transformers skips the cross layers when there is no image
        {
            Timed tm(c, s, KC_LN);
            HIP_TRY(c, launch_mllama_rmsnorm(t->x.p, L.ln1, t->h.p, M, D, t->eps, s));
        }
        if (!L.cross) {
            if ((r = ml_gemm(c, s, EPI_BIAS, t->h.p, L.qkv_w, M, D + 2 * KV, D, t->zeros, t->qkv.p, nullptr))) return r;
            {
                Timed tm(c, s, KC_LN);
                HIP_TRY(c, launch_mllama_rope(t->qkv.p, t->rope_cos, t->rope_sin, M, H + KVH, D + 2 * KV, S, s));
            }
            Timed tm(c, s, KC_ATTN);
            HIP_TRY(c, launch_mllama_self_attn(t->qkv.p, t->att.p, (const int32_t*)t->len.p, m, S, H, KVH, s));
        } else {
            if ((r = ml_gemm(c, s, EPI_BIAS, t->h.p, L.qkv_w, M, D, D, t->zeros, t->qkv.p, nullptr))) return r;
            if ((r = ml_gemm(c, s, EPI_BIAS, t->vis.p, L.kv_w, m * Nk, 2 * KV, D, t->zeros, t->kv.p, nullptr))) return r;
            {
                Timed tm(c, s, KC_LN);
                HIP_TRY(c, launch_mllama_headnorm(t->qkv.p, L.qn, M, H, D, 0, t->eps, s));
                HIP_TRY(c, launch_mllama_headnorm(t->kv.p, L.kn, (int64_t)m * Nk, KVH, 2 * KV, 0, t->eps, s));
            }
            Timed tm(c, s, KC_ATTN);
            HIP_TRY(c, launch_mllama_cross_attn(t->qkv.p, t->kv.p, (const uint8_t*)t->xm.p, t->att.p, (float*)t->cross_ws.p, m, S, H, KVH, tiles, tokens, s));
        }
        if ((r = ml_gemm(c, s, EPI_BIAS_RES, t->att.p, L.o_w, M, D, D, t->zeros, t->x.p, t->x.p))) return r;
        {
            Timed tm(c, s, KC_LN);
            HIP_TRY(c, launch_mllama_rmsnorm(t->x.p, L.ln2, t->h.p, M, D, t->eps, s));
        }
        if ((r = ml_gemm(c, s, EPI_BIAS, t->h.p, L.gu_w, M, 2 * I, D, t->zeros, t->gu.p, nullptr))) return r;
        {
            Timed tm(c, s, KC_LN);
            HIP_TRY(c, launch_mllama_silu_mul(t->gu.p, t->act.p, L.cross ? (const uint8_t*)t->rowzero.p : nullptr, M, I, s));
        }
        if ((r = ml_gemm(c, s, EPI_BIAS_RES, t->act.p, L.down_w, M, D, I, t->zeros, t->x.p, t->x.p))) return r;
    }
    Timed tm(c, s, KC_POOL);
    HIP_TRY(c, launch_mllama_pool(t->x.p, t->norm, (const int32_t*)t->len.p, m, S, D, t->eps, emb_f32, emb_bf16, s));
    return MME_OK;
}

// stages chunk [s0, s0 + m) of the call's integers; the host arrays are the caller's (ids, len) or the call's locals (xm, rowzero)
int stage_chunk(mme_ctx* c, MllamaDev* t, const int32_t* ids, const int32_t* len, const std::vector<uint8_t>& xm, const std::vector<uint8_t>& rowzero,
                bool vision, int s0, int m, int S, hipStream_t s) {
    HIP_TRY(c, hipMemcpyAsync(t->ids.p, ids + (size_t)s0 * S, (size_t)m * S * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(t->len.p, len + s0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (vision && t->ncross) {
        HIP_TRY(c, hipMemcpyAsync(t->xm.p, xm.data() + (size_t)s0 * S, (size_t)m * S, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(t->rowzero.p, rowzero.data() + (size_t)s0 * S, (size_t)m * S, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));  // the host arrays may be released, and the next chunk reuses the device buffers
    return MME_OK;
}

int chunk_of(const mme_ctx* c, int n) {
    const int per = c->chunk >= ML_CHUNK ? ML_CHUNK : (c->chunk < 1 ? 1 : c->chunk);
    return n < per ? n : per;
}

}  // namespace

extern "C" {

int mme_load_mllama_lm(mme_ctx* c, const mme_mllama_lm_weights* w) {
    int r;
    if ((r = validate_mllama(c, w, "mme_load_mllama_lm"))) return r;
    return load_mllama(c, w, HostPrep{c}, "mme_load_mllama_lm");
}

int mme_load_mllama_lm_as(mme_ctx* c, const mme_mllama_lm_weights* w, int dtype, void* stream) {
    int r;
    if ((r = validate_mllama(c, w, "mme_load_mllama_lm_as"))) return r;
    if ((r = check_load_dtype(c, dtype, "mme_load_mllama_lm_as"))) return r;
    return load_mllama(c, w, DevPrep(c, dtype, stream, "mme_load_mllama_lm_as"), "mme_load_mllama_lm_as");
}

int mme_mllama_lm_info(mme_ctx* c, int32_t out[12]) {
    if (!c || !out) return fail(c, MME_E_ARG, "mme_mllama_lm_info: null argument");
    for (int i = 0; i < 12; ++i) out[i] = 0;
    const MllamaDev* t = c->mllama;
    if (!t || !t->loaded) return MME_OK;
    const int32_t v[12] = {1, t->hidden, t->heads, t->kv_heads, t->inter, t->layers, t->ncross, t->vocab, t->vision_dim, t->image_token, t->rope_type,
                           (int32_t)c->mllama_alloc_lo};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return MME_OK;
}

int mme_mllama_lm_forward(mme_ctx* c, const int32_t* ids_host, const int32_t* len_host, int n, int S, const uint16_t* vision, int tiles, int tokens,
                          const int32_t* num_tiles_host, const uint8_t* xmask_host, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    const char* who = "mme_mllama_lm_forward";
    if (!c) return MME_E_ARG;
    MllamaDev* t = c->mllama;
    if (!t || !t->loaded) return fail(c, MME_E_STATE, "%s: call mme_load_mllama_lm first", who);
    if (n < 0 || (n > 0 && (!ids_host || !len_host))) return fail(c, MME_E_ARG, "%s: null ids / len or n < 0", who);
    if (S < 1 || S > MLLAMA_MAX_S) return fail(c, MME_E_ARG, "%s: S = %d; supported: 1..%d", who, S, MLLAMA_MAX_S);
    if (!emb_f32 && !emb_bf16) return fail(c, MME_E_ARG, "%s: needs emb_f32 or emb_bf16", who);
    if (!aligned16(emb_f32) || !aligned16(emb_bf16) || !aligned16(vision)) return fail(c, MME_E_ARG, "%s: device pointers must be 16-byte aligned", who);
    const bool vis = vision != nullptr;
    if (vis) {
        if (tiles < 1 || tiles > ML_MAX_TILES) return fail(c, MME_E_ARG, "%s: tiles = %d; supported: 1..%d", who, tiles, ML_MAX_TILES);
        if (tokens < 1 || tokens > ML_MAX_TOKENS) return fail(c, MME_E_ARG, "%s: tokens = %d; supported: 1..%d", who, tokens, ML_MAX_TOKENS);
        if (n > 0 && !xmask_host && !num_tiles_host) return fail(c, MME_E_ARG, "%s: vision rows need xmask_host or num_tiles_host", who);
    }
    if (n == 0) return MME_OK;
    std::vector<uint8_t> xm, rowzero;
    int r;
    if ((r = scan_sequences(c, who, t, ids_host, len_host, n, S, vis, tiles, num_tiles_host, xmask_host, xm, rowzero))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int cap = chunk_of(c, n), Nk = vis ? tiles * tokens : 0;
    if ((r = ensure_lm_workspace(c, t, cap, S, vis, Nk))) return r;
    const size_t D = (size_t)t->hidden;
    for (int s0 = 0; s0 < n; s0 += cap) {
        const int m = n - s0 < cap ? n - s0 : cap;
        if ((r = stage_chunk(c, t, ids_host, len_host, xm, rowzero, vis, s0, m, S, s))) return r;
        const bf16_t* st = vis ? (const bf16_t*)vision + (size_t)s0 * Nk * t->vision_dim : nullptr;
        if ((r = lm_chunk(c, t, m, S, st, tiles, tokens, emb_f32 ? emb_f32 + (size_t)s0 * D : nullptr, emb_bf16 ? (bf16_t*)emb_bf16 + (size_t)s0 * D : nullptr, s)))
            return r;
    }
    return MME_OK;
}

int mme_mllama_embed(mme_ctx* c, const float* pixel_values, const int32_t* aspect_ids_host, const int32_t* num_tiles_host, int n, const int32_t* ids_host,
                     const int32_t* len_host, int S, const uint8_t* xmask_host, float* emb_f32, uint16_t* emb_bf16, void* stream) {
    const char* who = "mme_mllama_embed";
    if (!c) return MME_E_ARG;
    MllamaDev* t = c->mllama;
    if (!t || !t->loaded) return fail(c, MME_E_STATE, "%s: call mme_load_mllama_lm first", who);
    const void *tx, *tinter;
    int ni;
    int64_t istride;
    int r;
    if ((r = tile_vit_states(c, who, &tx, &tinter, &ni, &istride))) return r;
    if (t->vision_dim != 1280 * (1 + ni))
        return fail(c, MME_E_STATE, "%s: the language tower's vision_dim = %d, the tile tower's output has %d features", who, t->vision_dim, 1280 * (1 + ni));
    if (n < 0 || (n > 0 && (!pixel_values || !aspect_ids_host || !num_tiles_host || !ids_host || !len_host))) return fail(c, MME_E_ARG, "%s: null argument or n < 0", who);
    if (S < 1 || S > MLLAMA_MAX_S) return fail(c, MME_E_ARG, "%s: S = %d; supported: 1..%d", who, S, MLLAMA_MAX_S);
    if (!emb_f32 && !emb_bf16) return fail(c, MME_E_ARG, "%s: needs emb_f32 or emb_bf16", who);
    if (!aligned16(emb_f32) || !aligned16(emb_bf16)) return fail(c, MME_E_ARG, "%s: device pointers must be 16-byte aligned", who);
    if (n == 0) return MME_OK;
    for (int i = 0; i < n; ++i)  // every image before the first launch: a refusal leaves no chunk's rows written
        if (aspect_ids_host[i] < 1 || aspect_ids_host[i] > 8 || num_tiles_host[i] < 1 || num_tiles_host[i] > ML_MAX_TILES)
            return fail(c, MME_E_ARG, "%s: image %d has aspect-ratio id %d / %d tiles (ids 1..8, tiles 1..4)", who, i, aspect_ids_host[i], num_tiles_host[i]);
    std::vector<uint8_t> xm, rowzero;
    if ((r = scan_sequences(c, who, t, ids_host, len_host, n, S, true, ML_MAX_TILES, num_tiles_host, xmask_host, xm, rowzero))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int cap = chunk_of(c, n), Nk = ML_MAX_TILES * ML_MAX_TOKENS;
    if ((r = ensure_lm_workspace(c, t, cap, S, true, Nk))) return r;
    if ((r = ensure(c, t->states, (size_t)cap * Nk * t->vision_dim * 2))) return r;
    const size_t D = (size_t)t->hidden;
    for (int s0 = 0; s0 < n; s0 += cap) {
        const int m = n - s0 < cap ? n - s0 : cap;
        // one pass of the tile tower (m <= its images per pass), no output asked for: the states stay in its buffers
        if ((r = mme_tile_vit_forward(c, pixel_values + (size_t)s0 * 4 * 3 * 560 * 560, aspect_ids_host + s0, num_tiles_host + s0, m, nullptr, nullptr, nullptr, stream)))
            return r;
        if ((r = tile_vit_states(c, who, &tx, &tinter, &ni, &istride))) return r;  // the pass may have grown the buffers
        {
            Timed tm(c, s, KC_POOL);
            HIP_TRY(c, launch_mllama_tile_states(tx, tinter, ni, istride, t->states.p, (int64_t)m * Nk, s));
        }
        if ((r = stage_chunk(c, t, ids_host, len_host, xm, rowzero, true, s0, m, S, s))) return r;
        if ((r = lm_chunk(c, t, m, S, t->states.p, ML_MAX_TILES, ML_MAX_TOKENS, emb_f32 ? emb_f32 + (size_t)s0 * D : nullptr,
                          emb_bf16 ? (bf16_t*)emb_bf16 + (size_t)s0 * D : nullptr, s)))
            return r;
    }
    return MME_OK;
}

int mme_mllama_apply(mme_ctx* c, int op, const mme_mllama_apply_args* a, void* stream) {
    const char* who = "mme_mllama_apply";
    if (int r = hook_args(c, who, a, op, 7)) return r;
    const HookCheck h{c, who, op};
    const char* bad = nullptr;
    const bool by_rows = op <= 4;
    const int64_t count = by_rows ? a->rows : a->n;
    const int64_t count_max = by_rows ? (1 << 22) : 65535;
    if (count < 0 || count > count_max) return fail(c, MME_E_ARG, "%s: op %d: %s = %lld outside 0..%lld", who, op, by_rows ? "rows" : "n", (long long)count, (long long)count_max);
    if (op == 0 || op == 1 || op == 4 || op == 5) {
        if (a->d < 8 || (a->d % 8) != 0 || a->d > 16384) return fail(c, MME_E_ARG, "%s: op %d: d = %d; supported: multiples of 8 in 8..16384", who, op, a->d);
    }
    if (op == 3 || op >= 5) {
        if (a->S < 1 || a->S > MLLAMA_MAX_S) return fail(c, MME_E_ARG, "%s: op %d: S = %d; supported: 1..%d", who, op, a->S, MLLAMA_MAX_S);
    }
    if (op == 2 || op == 3) {
        if (a->heads < 1 || a->col0 < 0 || (a->col0 % 8) != 0 || (a->ld % 8) != 0 || (op == 3 && a->col0 != 0) || (int64_t)a->col0 + (int64_t)a->heads * MLLAMA_DH > a->ld)
            return fail(c, MME_E_ARG, "%s: op %d: heads = %d, col0 = %d, ld = %lld; supported: heads >= 1, col0 and ld multiples of 8 (col0 = 0 for op 3), col0 + heads * 128 <= ld",
                        who, op, a->heads, a->col0, (long long)a->ld);
    }
    if (op >= 6 && (a->heads > ML_MAX_HEADS || !group_built(a->heads, a->kv_heads)))
        return fail(c, MME_E_ARG, "%s: op %d: heads = %d, kv_heads = %d; supported: heads <= %d, heads / kv_heads in {1, 2, 4, 8}", who, op, a->heads, a->kv_heads, ML_MAX_HEADS);
    if (op == 7 && (a->tiles < 1 || a->tiles > ML_MAX_TILES || a->tokens < 1 || a->tokens > ML_MAX_TOKENS))
        return fail(c, MME_E_ARG, "%s: op 7: tiles = %d, tokens = %d; supported: 1..%d, 1..%d", who, a->tiles, a->tokens, ML_MAX_TILES, ML_MAX_TOKENS);
    switch (op) {
        case 0:
            if (!vec16(a->tok) || !vec16(a->x) || !a->ids_host) bad = "tok, x non-null and 16-byte aligned, ids_host non-null";
            else if (a->vocab < 1 || a->vocab > ML_MAX_ROWS) return fail(c, MME_E_ARG, "%s: op 0 needs 1 <= vocab <= %d", who, ML_MAX_ROWS);
            break;
        case 1: if (!vec16(a->x) || !vec16(a->y) || !vec16(a->w)) bad = "x, y, w non-null and 16-byte aligned"; break;
        case 2: if (!vec16(a->x) || !vec16(a->w)) bad = "x, w non-null and 16-byte aligned"; break;
        case 3: if (!vec16(a->x) || !vec16(a->cos) || !vec16(a->sin)) bad = "x, cos, sin non-null and 16-byte aligned"; break;
        case 4: if (!vec16(a->x) || !vec16(a->y)) bad = "x, y non-null and 16-byte aligned"; break;
        case 5:
            if (!vec16(a->x) || !vec16(a->w) || !a->len_host) bad = "x, w non-null and 16-byte aligned, len_host non-null";
            else if (int r = h.out_pair(a->emb_f32, a->emb_bf16, "emb_f32", "emb_bf16")) return r;
            break;
        case 6: if (!vec16(a->x) || !vec16(a->y) || !a->len_host) bad = "x, y non-null and 16-byte aligned, len_host non-null"; break;
        default: if (!vec16(a->x) || !vec16(a->y) || !vec16(a->kv) || !a->xmask_host) bad = "x, y, kv non-null and 16-byte aligned, xmask_host non-null"; break;
    }
    if (bad) return h.needs(bad);
    if (op == 0)
        for (int64_t i = 0; i < count; ++i)
            if (a->ids_host[i] < 0 || a->ids_host[i] >= a->vocab)
                return fail(c, MME_E_ARG, "%s: op 0: ids_host[%lld] = %d outside 0..vocab-1 = 0..%d", who, (long long)i, a->ids_host[i], a->vocab - 1);
    if (op == 5 || op == 6)
        for (int b = 0; b < a->n; ++b)
            if (a->len_host[b] < 1 || a->len_host[b] > a->S) return fail(c, MME_E_ARG, "%s: op %d: len_host[%d] = %d outside 1..S = 1..%d", who, op, b, a->len_host[b], a->S);
    if (op == 7)
        for (int64_t i = 0; i < (int64_t)a->n * a->S; ++i)
            if (a->xmask_host[i] >= (1 << a->tiles))
                return fail(c, MME_E_ARG, "%s: op 7: xmask_host[%lld] = 0x%x; supported: below 1 << tiles = 0x%x", who, (long long)i, a->xmask_host[i], 1 << a->tiles);
    if (count == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int r;
    if ((r = mllama_dev(c, who))) return r;
    MllamaDev* t = c->mllama;
    const void* ints = nullptr;
    if (op == 0 || op == 5 || op == 6 || op == 7) {
        const void* src = op == 0 ? (const void*)a->ids_host : op == 7 ? (const void*)a->xmask_host : (const void*)a->len_host;
        const size_t bytes = op == 0 ? (size_t)count * 4 : op == 7 ? (size_t)a->n * a->S : (size_t)a->n * 4;
        if ((r = ensure(c, t->apply_ints, bytes))) return r;
        HIP_TRY(c, hipMemcpyAsync(t->apply_ints.p, src, bytes, hipMemcpyHostToDevice, s));
        ints = t->apply_ints.p;
    }
    switch (op) {
        case 0: HIP_TRY(c, launch_mllama_gather(a->tok, (const int32_t*)ints, a->x, count, a->d, s)); break;
        case 1: HIP_TRY(c, launch_mllama_rmsnorm(a->x, a->w, a->y, count, a->d, a->eps, s)); break;
        case 2: HIP_TRY(c, launch_mllama_headnorm(a->x, a->w, count, a->heads, a->ld, a->col0, a->eps, s)); break;
        case 3: HIP_TRY(c, launch_mllama_rope(a->x, a->cos, a->sin, count, a->heads, a->ld, a->S, s)); break;
        case 4: HIP_TRY(c, launch_mllama_silu_mul(a->x, a->y, a->rowzero, count, a->d, s)); break;
        case 5: HIP_TRY(c, launch_mllama_pool(a->x, a->w, (const int32_t*)ints, a->n, a->S, a->d, a->eps, a->emb_f32, a->emb_bf16, s)); break;
        case 6: HIP_TRY(c, launch_mllama_self_attn(a->x, a->y, (const int32_t*)ints, a->n, a->S, a->heads, a->kv_heads, s)); break;
        default: {
            if ((r = ensure(c, t->cross_ws, mllama_cross_workspace_floats(a->n, a->S, a->heads, a->tiles * a->tokens) * sizeof(float)))) return r;
            HIP_TRY(c, launch_mllama_cross_attn(a->x, a->kv, (const uint8_t*)ints, a->y, (float*)t->cross_ws.p, a->n, a->S, a->heads, a->kv_heads, a->tiles, a->tokens, s));
            break;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // extern "C"
