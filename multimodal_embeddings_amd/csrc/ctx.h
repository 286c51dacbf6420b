// Private to the library: the context behind `mme_ctx*` and the helpers the C-ABI translation units share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mme.h"
#include "common.h"
#include "kernels.h"

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// The ten prepared buffers of one transformer block in the form every tower runs (encoder_pass.h): LayerNorm folded into
// the consuming GEMM, W' = bf16(W * gamma), colsum = sum_k W', b' = b + W . beta
struct BlockW {
    bf16_t* qkv_wf;
    float *qkv_cs, *qkv_bf;
    bf16_t* o_w;
    float* o_b;
    bf16_t* fc1_wf;
    float *fc1_cs, *fc1_bf;
    bf16_t* fc2_w;
    float* fc2_b;
};

// a block of the image towers: the folded form, and the unfolded tensors that only the LayerNorm-kernel mode (ln_mode 0) reads
struct LayerDev {
    BlockW w;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    bf16_t *qkv_w, *fc1_w;
    float *qkv_b, *fc1_b;
};

// The ViT @224 geometry a context runs: that of the weights it was loaded with, ViT-B/16 before any load.
// Supported set (validate_vit_weights, weight_load.hip): image 224, heads of 64, hidden 384 / 768 / 1024, mlp % 64 == 0 and
// <= 8192, 1..64 layers, and a patch size and class token that make an image layout of layouts.h: patch 16 (197 tokens; 196
// under no_cls: SigLIP), patch 32 (50), patch 14 (257; DINOv2 only; the im2col row of 588 is padded to 640, a multiple of 64).
// What a layout is -- its kernels, heads, query blocks, pooled row -- is read from layout(), never spelled out per tower.
struct VitGeom {
    int hidden = VIT_D, layers = VIT_L, heads = VIT_H, mlp = VIT_F;
    int patch = VIT_PATCH;
    bool no_cls = false;
    int np() const { return (VIT_IMG / patch) * (VIT_IMG / patch); }  // patches per crop: 196, 49 or 256
    int tokens() const { return np() + (no_cls ? 0 : 1); } // 197, 50 or 257; 196 without a class token
    const TokenLayout& layout() const { return *find_layout(tokens()); }  // the loaders admit no other geometry
    int patch_elems() const { return 3 * patch * patch; }  // the checkpoint's im2col row: 768, 3072 or 588
    int patch_dim() const { return (patch_elems() + 63) & ~63; }  // K of the patch-embed GEMM: 768, 3072 or 640 (the row's patch_dim)
    size_t crop_values() const { return (size_t)np() * patch_dim(); }  // bf16 values of one crop's patch matrix: 150 528 at patch 16 and 32, 163 840 at patch 14
};

enum KClass { KC_PRE = 0, KC_GEMM = 1, KC_LN = 2, KC_ATTN = 3, KC_POOL = 4, KC_COS = 5, KC_PAGE = 6, KC_CLUSTER = 7, KC_NEIGH = 8, KC_COMM = 9 };

struct EventPair {
    hipEvent_t a, b;
    int cls;
};

struct TileVitDev;  // capi_tilevit.hip
struct TextDev;     // capi_text.hip
struct MllamaDev;   // capi_mllama.hip

struct mme_ctx {
    int device = 0;
    std::string err;
    bool loaded = false;
    float ln_eps = 1e-12f;
    int chunk = 4096;
    int gemm_variant = 0;
    int ln_mode = 2;  // 0 LayerNorm kernel, 1 folded into the GEMMs + one statistics pass over x, 2 folded + partial sums from the producing epilogue
    int neigh_mode = 0;  // K12: 0 by size, 1 cosine block through the workspace, 2 fused candidate lists
    // weights
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;  // size of allocs[i] (mme_weights_fingerprint)
    size_t vit_alloc_lo = 0, vit_alloc_hi = 0;  // allocs[lo, hi): the ViT weights (a second mme_load_vit* frees exactly these)
    VitGeom geom;
    float *cls = nullptr, *pos = nullptr, *patch_b = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    bf16_t* patch_w = nullptr;
    std::vector<LayerDev> layer;  // geom.layers of them
    // CLIP image tower (mme_load_clip*; all off / null after mme_load_vit*): a LayerNorm over every token row before layer 0,
    // QuickGELU in the MLP, a bias-free projection of the pooled, LayerNormed row
    bool clip = false;         // the last load was a CLIP load (mme_encoder_info); pre_g / pre_b are set
    int act = 0;               // 0 erf-GELU, 1 QuickGELU, 2 tanh-GELU (SigLIP)
    int proj_dim = 0;          // 0: no projection (the embedding is the L2-normalised post_layernorm row)
    float *pre_g = nullptr, *pre_b = nullptr;
    bf16_t* proj_w = nullptr;  // [proj_dim, hidden]
    // SigLIP image tower (mme_load_siglip*; off / null after every other load): no class token, tanh-GELU (act 2), and the
    // attention-pooling head in place of the pooled token.  `head` is a block in the towers' form whose "QKV" is the K | V
    // projection [2 D, D] of the head's in_proj with post_layernorm (lnf_g, lnf_b) folded in, whose o_w / o_b is out_proj
    // and whose ln2 / fc1 / fc2 are the head's layernorm and MLP; head_q [D] f32 is the constant query
    // (probe . W_q^T + b_q) dh^-0.5 log2 e.  head.ln1_g / ln1_b are not set (ln_mode 0 normalises with lnf_g / lnf_b).
    bool siglip = false;
    bool dinov2 = false;  // the last load was a DINOv2 load (mme_encoder_info kind 3): patch 14, LayerScale folded into o_w / o_b / fc2_w / fc2_b
    LayerDev head{};
    float* head_q = nullptr;
    float* lut = nullptr;  // [3,256]
    NormAffine norm_aff{};  // the same mapping as one fma per value where that is bit-exact after the bf16 rounding (set_lut)
    int resize_rule = MME_RESIZE_FIT_PAD;  // mme_set_resize_rule: how mme_preprocess / mme_embed make 224 x 224 pixels; no load changes it
    mme_resize_spec resize_spec{};  // mme_set_resize_spec: the rule's parameters while resize_rule == MME_RESIZE_SPEC
    // workspace (sized for `chunk` crops)
    int ws_chunk = 0, ws_hidden = 0, ws_mlp = 0, ws_tokens = 0;  // what the workspace below was sized for
    DevBuf attn_guard;      // int[max(64, layers)]: one guard word per layer of a pass (encoder_pass.h, reset_attn_guards)
    DevBuf attn_apply;      // mme_attention_apply: its own guard word (int 0), the tile counts from int 16 on
    bool prune_last = false;  // mme_set_forward_pruning
    int pool_mode = MME_POOL_TOKEN;  // mme_set_pooling; every load sets it back to MME_POOL_TOKEN
    DevBuf pool_grids;               // int32 [n, 2]: the covered grids of a call (mme_vit_forward_grids) or of a chunk (the pixel path)
    std::vector<int32_t> h_pool_grids;  // host staging of a chunk's grids
    int zigzag = 1;           // EncoderPass::zigzag of the image towers (image_tower.hip): 1 = consecutive kernels walk the rows in opposite directions, 2 = attention only
    int attn_mode = 1;      // mme_set_attention_mode: 0 exact, 1 fast (guarded), 2 fast with the guard forced (tests)
    DevBuf x, hbuf, qkv, att, mlp, stats, lnpart, patches, tmp, htab, crops, hwork, page_ws, cluster_ws, neigh_ws, zero_bias;
    DevBuf retiled;        // patch 32 / 14: the retiled [chunk * 49, 3072] / [chunk * 256, 640] matrix of mme_embed (`patches` stages K1's patch-16 matrix)
    DevBuf pooled, projf;  // CLIP tail: bf16 [chunk, hidden] post_layernorm rows, f32 [chunk, proj_dim] projected rows
                           // SigLIP tail: pooled = bf16 [2][chunk, hidden] (map_pool's rows, then the head's residual rows)
    // host staging for crop tables
    std::vector<CropDesc> h_crops;
    std::vector<ClipCropDesc> h_clip_crops;
    std::vector<HWork> h_work;
    // profiling
    bool prof = false;
    std::vector<EventPair> events;
    size_t events_used = 0;
    // tile-ViT encoder option
    TileVitDev* tv = nullptr;
    // CLIP text tower (capi_text.hip): coexists with the image tower; allocs[text_alloc_lo, text_alloc_hi) are its weights
    TextDev* text = nullptr;
    size_t text_alloc_lo = 0, text_alloc_hi = 0;
    // Mllama language tower (capi_mllama.hip): coexists with every other tower; allocs[mllama_alloc_lo, mllama_alloc_hi) are its weights
    MllamaDev* mllama = nullptr;
    size_t mllama_alloc_lo = 0, mllama_alloc_hi = 0;
};

// Frees allocs[lo, hi) (the caller has drained the device) and takes them out of the tables; every other tower's range (the
// ViT's, the text tower's, the Mllama language tower's) moves down with its buffers when it sits behind.  Afterwards
// lo == hi == allocs.size(): the buffers the load creates next are the new range.
inline void release_alloc_range(mme_ctx* c, size_t& lo, size_t& hi) {
    const size_t n = hi - lo, end = hi;
    if (n) {
        for (size_t i = lo; i < hi; ++i) (void)hipFree(c->allocs[i]);
        c->allocs.erase(c->allocs.begin() + lo, c->allocs.begin() + hi);
        c->alloc_bytes.erase(c->alloc_bytes.begin() + lo, c->alloc_bytes.begin() + hi);
        size_t* ranges[3][2] = {{&c->vit_alloc_lo, &c->vit_alloc_hi}, {&c->text_alloc_lo, &c->text_alloc_hi}, {&c->mllama_alloc_lo, &c->mllama_alloc_hi}};
        for (auto& r : ranges)
            if (r[0] != &lo && *r[0] >= end) {
                *r[0] -= n;
                *r[1] -= n;
            }
    }
    lo = hi = c->allocs.size();
}

int fail(mme_ctx* c, int code, const char* fmt, ...);
// width of the rows mme_vit_forward / mme_embed write ([y_0 | m] under MME_POOL_CLS_MEAN, which only a tower without projection takes)
inline int embed_dim(const mme_ctx* c) { return c->proj_dim ? c->proj_dim : (c->pool_mode == MME_POOL_CLS_MEAN ? 2 : 1) * c->geom.hidden; }
// The covered grids (R, C) of n crops under the context's patch size and resize rule -> out int32 [n, 2] (capi.hip, mme_pool_grids):
// the fit-and-pad rule covers ceil(new / patch) patches per axis, every rule that fills the canvas all of them.  A crop outside
// 1..8000 is MME_E_ARG in `who`'s name.
int pool_grids_host(mme_ctx* c, const char* who, const int32_t* hw, int n, int32_t* out);

#define HIP_TRY(c, expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail((c), MME_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int ensure(mme_ctx* c, DevBuf& b, size_t bytes);

// ---- The checks the single-launch *_apply hooks share, each written once.  who: the hook; op: its op code; L: the layout the
// hook runs (layouts.h).  A refusal is MME_E_ARG in the hook's own words, 0 is "go on".
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool vec16(const void* p) { return p && aligned16(p); }
struct HookCheck {
    mme_ctx* c;
    const char* who;
    int op;
    int needs(const char* what) const { return fail(c, MME_E_ARG, "%s: op %d needs %s", who, op, what); }
    int crops(int n) const { return n < 0 || n > (1 << 20) ? fail(c, MME_E_ARG, "%s: n = %d outside 0..2^20", who, n) : MME_OK; }
    int width(int d) const { return vit_width_built(d) ? MME_OK : fail(c, MME_E_ARG, "%s: op %d is built for d == 384, d == 768 and d == 1024 (d = %d)", who, op, d); }
    int heads(const TokenLayout& L, int h) const { return L.has_heads(h) ? MME_OK : fail(c, MME_E_ARG, "%s: op %d is built for heads == %d, %d and %d (heads = %d)", who, op, L.heads[0], L.heads[1], L.heads[2], h); }
    // embed rows: the width, then every tensor (cls among them exactly when the layout has a class row)
    int embed_rows(const TokenLayout& L, int d, const void* acc, const void* bias, const void* pos, const void* cls, const void* x) const {
        if (int r = width(d)) return r;
        if (vec16(acc) && vec16(bias) && vec16(pos) && (!L.cls || vec16(cls)) && vec16(x)) return MME_OK;
        return needs(L.cls ? "acc, bias, pos, cls, x non-null and 16-byte aligned" : "acc, bias, pos, x non-null and 16-byte aligned");
    }
    // the pooled LayerNorm: its input, its token, and the two outputs (named nf, nb) of the form with the L2 step
    int ln_in(const void* x, const void* gamma, const void* beta) const { return vec16(x) && vec16(gamma) && vec16(beta) ? MME_OK : needs("x, gamma, beta non-null and 16-byte aligned"); }
    int tok(const TokenLayout& L, int t) const { return t < 0 || t >= L.tokens ? fail(c, MME_E_ARG, "%s: op %d needs 0 <= tok <= %d", who, op, L.tokens - 1) : MME_OK; }
    int out_pair(const void* f32, const void* bf16, const char* nf, const char* nb) const {
        if (!f32 && !bf16) return fail(c, MME_E_ARG, "%s: op %d needs %s or %s", who, op, nf, nb);
        return aligned16(f32) && aligned16(bf16) ? MME_OK : fail(c, MME_E_ARG, "%s: op %d needs %s and %s 16-byte aligned", who, op, nf, nb);
    }
};
// what every hook refuses first: no context, no args struct, an op code outside 0..last
inline int hook_args(mme_ctx* c, const char* who, const void* a, int op, int last) {
    if (!c) return MME_E_ARG;
    if (!a) return fail(c, MME_E_ARG, "%s: null argument", who);
    return op < 0 || op > last ? fail(c, MME_E_ARG, "%s: op %d outside 0..%d", who, op, last) : MME_OK;
}

// K1 (capi.hip) of n <= chunk crops under the context's resize rule -> patches bf16 [n * 196, 768], the patch-16 matrix
int preprocess_chunk(mme_ctx* c, const uint8_t* pix, const int64_t* offs, const int32_t* hw, int n, bf16_t* patches, hipStream_t s);
// f32 -> bf16, round to nearest even, NaN kept quiet (bf16_rne_bits of weight_prep.hip is its device form, bit for bit)
inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// an f32 table value as both preparers store it: a NaN leaves as a quiet NaN (every other value unchanged, bit for bit)
inline float f32_quiet_nan(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) u |= 0x00400000u;
    memcpy(&f, &u, 4);
    return f;
}
void tile_vit_free(mme_ctx* c);
void text_free(mme_ctx* c);  // the text tower's record and workspace (its weights are in c->allocs)
void mllama_free(mme_ctx* c);  // the Mllama language tower's record and workspace (its weights are in c->allocs)
// the tile tower's states after a pass of <= 64 images (capi_tilevit.hip): x and the ni intermediate states, bf16 rows of 1280
// padded to 1608 per tile; MME_E_STATE in `who`'s name without a tile tower
int tile_vit_states(mme_ctx* c, const char* who, const void** x, const void** inter, int* ni, int64_t* inter_stride);

// ---- weight loading (weight_load.hip) ---------------------------------------------------------------------------------
// Each encoder's load is ONE sequence of prepared buffers (prepare_vit in weight_load.hip, prepare_tile in
// capi_tilevit.hip), written against the operations that the two preparers below share.  The sequence reads the caller's
// weights struct: through HostPrep its pointers are the caller's host f32 tensors, through DevPrep they are the device
// addresses of the staged checkpoint bytes (elements of `dt`).  Both produce the same bits
// (tests/test_gpu_checkpoint.py compares the fingerprints):
//   a factor is applied in f32, and rounded to f32, before anything else, and only where `scaled` says so;
//   bf16 rounding is nearest-even with NaN kept quiet;
//   the LayerNorm fold is W' = bf16(w * gamma), colsum = sum_k W' (of the ROUNDED values, so that r * (W'x - mu * colsum)
//   is exact algebra), bias' = b + sum_k w * beta (a null b counts as 0), both sums over k ascending in one f64
//   accumulator per row.
// Both register every prepared buffer in c->allocs / c->alloc_bytes, in creation order.
int check_load_dtype(mme_ctx* c, int dtype, const char* who);

// The host loops (f32 in): prepared on the CPU, one upload per buffer.  The kernels keep these loops' operations and their order.
struct HostPrep {
    mme_ctx* c;
    template <class Walk>
    int stage(Walk&&) { return MME_OK; }  // the tensors are read where the caller holds them
    int finish(int r) { return r; }
    // f32 table; `scaled`: every value times `scale` first
    int table(const void* src, size_t n, float scale, bool scaled, float** dst);
    // concatenated f32 table; the first part times `scale0` when `scaled0`
    int table_cat(const void* const* srcs, const size_t* n, int nsrc, float scale0, bool scaled0, float** dst);
    // up to three [rows_i, cols] matrices, row-wise, as bf16; the first part times `scale0` when `scaled0`
    int bf16(const void* const* srcs, const size_t* rows, int nsrc, size_t cols, float scale0, bool scaled0, bf16_t** dst);
    // LayerNorm folding for `y = W . LN(x) + b` of up to three row blocks
    int folded(const WpFoldSrc* srcs, const size_t* rows, int nsrc, size_t cols, const void* gamma, const void* beta, bf16_t** wf, float** cs, float** bf);
    // [rows, cols] -> bf16 [rows, cols_padded], zero columns behind
    int padded(const void* src, int rows, int cols, int cols_padded, bf16_t** dst);
    int zeros(size_t n, float** dst);
    // bf16 matrix with a per-row f32 factor: dst[n, k] = bf16_rne(f32(factor[n] * src[n, k])); cols a multiple of 8
    int rowscaled(const void* src, size_t rows, size_t cols, const void* factor, bf16_t** dst);
    // f32 table dst[i] = f32(factor[i] * src[i])
    int table_mul(const void* src, const void* factor, size_t n, float** dst);
};

// The checkpoint's bytes on the device for the duration of one load.  Two walks over the tensors with the same calls:
// the first (dry) sizes the buffer and leaves every pointer as it is, reserve() allocates it, the second copies and
// returns the device addresses (16-byte aligned).  release() waits for the stream and frees: nothing of it stays in the
// context.
struct WeightStage {
    char* base = nullptr;
    size_t total = 0, used = 0, esz;
    bool dry = true;
    hipStream_t s;
    hipError_t err = hipSuccess;
    WeightStage(int dt, hipStream_t s_) : esz(dt == MME_DT_F32 ? 4 : 2), s(s_) {}
    int reserve(mme_ctx* c);
    const void* put(const void* host, size_t n);
    void release();
};

// The kernels of weight_prep.hip on staged bytes of `dt` (f32, bf16 or f16): HostPrep's operations, launched on `s`.
struct DevPrep {
    mme_ctx* c;
    int dt;
    hipStream_t s;
    const char* who;  // the entry point, for the error texts
    WeightStage st;
    DevPrep(mme_ctx* c_, int dt_, void* stream, const char* who_) : c(c_), dt(dt_), s((hipStream_t)stream), who(who_), st(dt_, s) {}
    // walk(put) calls put(pointer, elements) for every tensor of a weights struct; afterwards the pointers are device addresses
    template <class Walk>
    int stage(Walk&& walk) {
        auto put = [this](const float*& p, size_t n) { p = (const float*)st.put(p, n); };
        walk(put);
        int r = st.reserve(c);
        if (r) return r;
        walk(put);
        if (st.err != hipSuccess) return fail(c, MME_E_HIP, "%s: copying the checkpoint's bytes to the device: %s", who, hipGetErrorString(st.err));
        return MME_OK;
    }
    // waits for the preparation, frees the staged bytes
    int finish(int r);
    int table(const void* src, size_t n, float scale, bool scaled, float** dst);
    int table_cat(const void* const* srcs, const size_t* n, int nsrc, float scale0, bool scaled0, float** dst);
    int bf16(const void* const* srcs, const size_t* rows, int nsrc, size_t cols, float scale0, bool scaled0, bf16_t** dst);
    int folded(const WpFoldSrc* srcs, const size_t* rows, int nsrc, size_t cols, const void* gamma, const void* beta, bf16_t** wf, float** cs, float** bf);
    int padded(const void* src, int rows, int cols, int cols_padded, bf16_t** dst);
    int zeros(size_t n, float** dst);
    // bf16 matrix with a per-row f32 factor: dst[n, k] = bf16_rne(f32(factor[n] * src[n, k])); cols a multiple of 8
    int rowscaled(const void* src, size_t rows, size_t cols, const void* factor, bf16_t** dst);
    // f32 table dst[i] = f32(factor[i] * src[i])
    int table_mul(const void* src, const void* factor, size_t n, float** dst);
};

struct Timed {
    mme_ctx* c;
    hipStream_t s;
    EventPair* ev = nullptr;
    Timed(mme_ctx* c_, hipStream_t s_, int cls);
    ~Timed();
};
