// Private to the library: the context behind `mme_ctx*` and the helpers the C-ABI translation units share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mme.h"
#include "common.h"
#include "kernels.h"

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct LayerDev {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    bf16_t *qkv_w, *o_w, *fc1_w, *fc2_w;
    float *qkv_b, *o_b, *fc1_b, *fc2_b;
    // LayerNorm folded into the consuming GEMM: W' = bf16(W * gamma), colsum = sum_k W', b' = b + W . beta
    bf16_t *qkv_wf, *fc1_wf;
    float *qkv_cs, *qkv_bf, *fc1_cs, *fc1_bf;
};

// The ViT/16 @224 geometry a context runs: that of the weights it was loaded with, ViT-B/16 before any load.
// Supported set (validate_vit_weights): image 224, patch 16, heads of 64, hidden 384 / 768 / 1024, mlp % 64 == 0 and
// <= 8192, 1..64 layers.
struct VitGeom {
    int hidden = VIT_D, layers = VIT_L, heads = VIT_H, mlp = VIT_F;
};

enum KClass { KC_PRE = 0, KC_GEMM = 1, KC_LN = 2, KC_ATTN = 3, KC_POOL = 4, KC_COS = 5, KC_PAGE = 6, KC_CLUSTER = 7, KC_NEIGH = 8, KC_COMM = 9 };

struct EventPair {
    hipEvent_t a, b;
    int cls;
};

struct TileVitDev;  // capi_tilevit.hip

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
    float* lut = nullptr;  // [3,256]
    NormAffine norm_aff{};  // the same mapping as one fma per value where that is bit-exact after the bf16 rounding (set_lut)
    // workspace (sized for `chunk` crops)
    int ws_chunk = 0, ws_hidden = 0, ws_mlp = 0;  // what the workspace below was sized for
    DevBuf attn_guard;      // int[64]: one guard word per layer of a pass (attention.hip, FAST form)
    DevBuf attn_apply;      // mme_attention_apply: its own guard word (int 0), the tile counts from int 16 on
    bool prune_last = false;  // mme_set_forward_pruning
    int zigzag = 1;           // forward_chunk: 1 = consecutive kernels walk the rows in opposite directions, 2 = attention only
    int attn_mode = 1;      // mme_set_attention_mode: 0 exact, 1 fast (guarded), 2 fast with the guard forced (tests)
    DevBuf x, hbuf, qkv, att, mlp, stats, lnpart, patches, tmp, htab, crops, hwork, page_ws, cluster_ws, neigh_ws, zero_bias;
    // host staging for crop tables
    std::vector<CropDesc> h_crops;
    std::vector<HWork> h_work;
    // profiling
    bool prof = false;
    std::vector<EventPair> events;
    size_t events_used = 0;
    // tile-ViT encoder option
    TileVitDev* tv = nullptr;
};

int fail(mme_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail((c), MME_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int ensure(mme_ctx* c, DevBuf& b, size_t bytes);
uint16_t f32_to_bf16_rne(float f);
int upload_f32(mme_ctx* c, const float* src, size_t n, float** dst);
// concatenates up to three [rows_i, cols] f32 matrices row-wise, converts to bf16, uploads; `scale` multiplies every value first
int upload_bf16(mme_ctx* c, const float* const* srcs, const size_t* rows, int nsrc, size_t cols, bf16_t** dst, float scale = 1.0f);
// LayerNorm folding for `y = W . LN(x) + b` (bs[i] may be null: no bias)
int upload_folded(mme_ctx* c, const float* const* ws, const float* const* bs, const size_t* rows, int nsrc, size_t cols, const float* gamma,
                  const float* beta, bf16_t** wf, float** cs, float** bf);
void tile_vit_free(mme_ctx* c);
// argument checks shared by mme_load_vit and mme_load_vit_as (`who` names the f32 loader in the messages of both): the
// geometry against the supported set, every tensor pointer.  Touches nothing in the context but its error text.
int validate_vit_weights(mme_ctx* c, const mme_vit_weights* w, const char* who);
// A load replaces what the context held: begin frees the previous ViT weights (after the device has drained), takes the
// new geometry and leaves the context unloaded; end marks the buffers allocated since as the ViT weights and, when
// `ok`, the context as loaded.  A load that fails in between leaves the context without weights.
int begin_vit_load(mme_ctx* c, const mme_vit_weights* w);
void end_vit_load(mme_ctx* c, bool ok);

// ---- device-side weight preparation (weight_prep.hip): the upload_* helpers above, from staged device bytes of `dt` ----
// hipMalloc registered in c->allocs / c->alloc_bytes
int alloc_weight(mme_ctx* c, size_t bytes, void** out);
// The checkpoint's bytes on the device for the duration of one load.  Two walks over the tensors with the same calls:
// the first (dry) sizes the buffer, reserve() allocates it, the second copies and returns the device addresses
// (16-byte aligned).  release() waits for the stream and frees: nothing of it stays in the context.
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
// dt -> f32 table, `scaled`: every value times `scale` first (upload_f32 / upload_scaled_f32)
int prep_table(mme_ctx* c, int dt, const void* src, size_t n, float scale, bool scaled, float** dst, hipStream_t s);
// upload_f32_cat; the first part times `scale0` when `scaled0`
int prep_table_cat(mme_ctx* c, int dt, const void* const* srcs, const size_t* n, int nsrc, float scale0, bool scaled0, float** dst, hipStream_t s);
// upload_bf16; the first part times `scale0` when `scaled0`
int prep_bf16(mme_ctx* c, int dt, const void* const* srcs, const size_t* rows, int nsrc, size_t cols, bf16_t** dst, float scale0, bool scaled0,
              hipStream_t s);
// upload_folded
int prep_folded(mme_ctx* c, int dt, const WpFoldSrc* srcs, const size_t* rows, int nsrc, size_t cols, const void* gamma, const void* beta, bf16_t** wf,
                float** cs, float** bf, hipStream_t s);

struct Timed {
    mme_ctx* c;
    hipStream_t s;
    EventPair* ev = nullptr;
    Timed(mme_ctx* c_, hipStream_t s_, int cls);
    ~Timed();
};
