/* mme.h -- C ABI of the MI355X-native region embed -> compare -> page-cluster engine.
 *
 * The reference (calhounpaul/multimodal_embeddings) has no FFI: its hot path is two
 * duck-typed Python objects (an `embedder` and a vector-store `collection`) plus two
 * free functions.  This header is the boundary a maintainer binds with
 * ctypes (INTEGRATION.md shows the stub); each entry point cites the reference
 * interface it replaces.  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - one mme_ctx per GPU / per process rank; not thread-safe (use one ctx per thread);
 *   - every function returns 0 on success or a negative MME_E_* code and never throws;
 *     mme_last_error(ctx) returns the message of the last failure;
 *   - "dev" pointers are device (HBM) pointers owned by the caller, "host" pointers are
 *     ordinary host memory; all launches are asynchronous on `stream` (a hipStream_t
 *     passed as void*; NULL = the default stream) unless the name ends in _sync;
 *   - ordering (held by tests/test_gpu_streams.py for every entry point): every step a result depends on -- kernels, memsets,
 *     copies, the first-call initialisation of context state -- is enqueued on `stream` and on no other, so outputs are
 *     complete once `stream` has reached the end of the call, whatever the null stream or any other stream is doing.  The
 *     context's scratch (crop descriptors, band lists, resampling tables, the cosine workspace K12 / K14 / K15 / K16 share, the
 *     guard words, the staging vectors on the host) is SHARED between calls: calls on one context must be ordered with respect
 *     to one another -- issued on the same stream, or on different streams with an event dependency from each call to the
 *     next.  Two calls back to back on one stream need no host synchronisation between them.  Calls on two streams with no
 *     dependency between them need two contexts;
 *   - caller HOST arrays (crop offsets and sizes, boxes, token ids, page offsets, init_rows, tile counts, aspect-ratio ids)
 *     are read before the call returns: the caller may overwrite or free them on return, while the device work is pending.
 *     Host OUTPUT arrays are complete on return (such entry points wait for `stream` and say so);
 *   - an entry point may make the host wait where its text says so, and when scratch has to grow: growing a buffer that
 *     already exists waits for the whole device before the old one is freed.  Steady-state calls of one shape do not wait;
 *   - bf16 = 16-bit brain float stored as uint16_t.
 */
#ifndef MME_H
#define MME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an export changes its signature, the meaning of an argument or the size of a caller-owned array.
 * 2 (round 3): mme_profile_read_sync takes the capacity of the caller's arrays (the class count is no longer part of
 *    the ABI); mme_set_ln_fusion's argument is a MODE (0 / 1 / 2, it was on / off in version 1); mme_tile_vit_weights
 *    carries the save point of the intermediate states; the experiment switches exist only in a
 *    -DMME_DIAG build; new exports mme_is_diag_build, mme_set_attention_mode, mme_attention_redone,
 *    mme_set_tile_order, mme_set_forward_pruning.  A binder checks `mme_abi_version() == MME_ABI_VERSION` right after dlopen. */
#define MME_ABI_VERSION 2

enum {
    MME_OK = 0,
    MME_E_ARG = -1,     /* bad argument (null pointer, size, alignment) */
    MME_E_STATE = -2,   /* call order (e.g. forward before load) */
    MME_E_HIP = -3,     /* HIP runtime / launch failure */
    MME_E_NOMEM = -4,
    MME_E_COMM = -5     /* RCCL missing or a collective failed */
};

typedef struct mme_ctx mme_ctx;

/* ---- lifetime ---------------------------------------------------------------------
 * Replaces MmE5MllamaEmbedder.__init__'s per-device replica set-up
 * (deprecated_package/embedder.py:42-84): one context per visible GPU. */
int mme_abi_version(void);
/* 1 when the library was built with -DMME_DIAG (libmme_diag.so): only then are the experiment switches of DESIGN.md
 * 4.5 (MME_ATTN_DEBUG, MME_TATTN_DEBUG) read from the environment.  The production library ignores them. */
int mme_is_diag_build(void);
int mme_create(int device, mme_ctx** out);
void mme_destroy(mme_ctx* ctx);
const char* mme_last_error(const mme_ctx* ctx); /* ctx may be NULL: creation errors */

/* ---- encoder weights --------------------------------------------------------------
 * Replaces `MllamaForConditionalGeneration.from_pretrained(...)` (embedder.py:75-80) for
 * the re-scoped ViT/16 encoder (ViT-S, ViT-B or ViT-L at 224 pixels).  Host f32 tensors in Hugging Face ViT layout
 * (transformers models/vit/modeling_vit.py): Linear weights are [out, in]; the patch
 * projection is [hidden, 3*patch*patch] in (c, ky, kx) order.  Values are rounded to
 * bf16 on upload (the reference runs the encoder in bf16, embedder.py:78).
 * Supported geometries: image_size 224, patch_size 16 or 32 (197 or 50 tokens; pos_emb [197 | 50, hidden], patch_w
 * [hidden, 768 | 3072]), heads of 64 (heads == hidden / 64), hidden 384, 768 or 1024,
 * mlp a multiple of 64 up to 8192, 1..64 layers, any ln_eps.  Anything else is MME_E_ARG with a text that names the
 * field, the value found and the supported values; nothing in the context changes then.
 * A context runs the geometry of its LAST successful load, ViT-B/16 (224/16/768/12/12/3072) before any: a second load
 * replaces the first whatever the two geometries are (the old weight buffers are freed once the device has drained, the
 * activation workspace regrows on the next pass).  A load that fails after validation leaves the context without
 * weights. */
typedef struct {
    const float *ln1_g, *ln1_b;
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;
    const float *ln2_g, *ln2_b;
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} mme_vit_layer;

typedef struct {
    int32_t image_size;  /* 224 */
    int32_t patch_size;  /* 16 or 32 */
    int32_t hidden;      /* 384, 768 or 1024 */
    int32_t layers;      /* 1..64 */
    int32_t heads;       /* hidden / 64 */
    int32_t mlp;         /* multiple of 64, <= 8192 */
    float ln_eps;        /* 1e-12 */
    const float* cls_token; /* [hidden] */
    const float* pos_emb;   /* [1 + (image/patch)^2, hidden] */
    const float* patch_w;   /* [hidden, 3*patch*patch] */
    const float* patch_b;   /* [hidden] */
    const float* lnf_g;     /* final LayerNorm */
    const float* lnf_b;
    const mme_vit_layer* layer; /* [layers] */
} mme_vit_weights;

int mme_load_vit(mme_ctx* ctx, const mme_vit_weights* w);
/* out[6] = image_size, patch_size, hidden, layers, heads, mlp of the context's encoder: what the last load brought,
 * ViT-B/16 before any.  mme_vit_forward / mme_embed write rows of `hidden`. */
int mme_vit_geometry(mme_ctx* ctx, int32_t out[6]);

/* The same load from a checkpoint's OWN element type, prepared on the device.  Replaces the `torch_dtype=bfloat16` read of
 * `from_pretrained` (embedder.py:75-80) for a checkpoint on local disk: every tensor pointer of `w` (and of its layer
 * array) points at HOST elements of `dtype` -- the struct fields keep their `const float*` type, cast the pointers.  The
 * raw bytes are copied to a device staging buffer (freed before the call returns, not part of the context).  The two loaders
 * run ONE sequence of prepared buffers with two preparers: mme_load_vit's host loops, and here kernels with the same
 * operations in the same order -- convert, scale the query rows, round to bf16, fold the LayerNorms with their f64 column
 * sums over k ascending -- so the buffers are BIT-IDENTICAL to mme_load_vit's on the same values widened to f32
 * (mme_weights_fingerprint compares two contexts).  A bf16 checkpoint is never inflated to f32 on the host.
 * Same validation and error texts as mme_load_vit.  Synchronises `stream` before returning: the host tensors may be
 * released right after. */
enum { MME_DT_F32 = 0, MME_DT_BF16 = 1, MME_DT_F16 = 2 };
int mme_load_vit_as(mme_ctx* ctx, const mme_vit_weights* w, int dtype, void* stream);

/* ---- CLIP ViT/16 image towers ------------------------------------------------------------------------------------------
 * Replaces `CLIPVisionModelWithProjection.from_pretrained(dir)(pixel_values).image_embeds` (or `CLIPVisionModel`'s
 * pooler_output when the checkpoint has no projection), L2-normalised, for the towers at this engine's geometry: 224
 * pixels, patch 16, heads of 64 (clip-vit-base-patch16 and its re-trainings).  The tower is the ViT forward above with
 * five differences (transformers models/clip/modeling_clip.py):
 *   - CLIPVisionEmbeddings: the patch convolution has no bias (`bias=False`): vit.patch_b may be NULL and is prepared as a
 *     table of zeros; vit.cls_token is class_embedding, vit.pos_emb is position_embedding.weight [197, hidden];
 *   - CLIPVisionTransformer.forward: `hidden_states = self.pre_layrnorm(hidden_states)` over every token row before
 *     layer 0 (pre_g, pre_b);
 *   - CLIPMLP: `self.activation_fn = ACT2FN[config.hidden_act]`: "quick_gelu" (act 1, x * sigmoid(1.702 x), activations.py
 *     QuickGELUActivation) for OpenAI weights, "gelu" (act 0) for the LAION conversions;
 *   - CLIPEncoderLayer: layer_norm1 / layer_norm2 with `eps=config.layer_norm_eps`, 1e-5 (vit.ln_eps);
 *   - CLIPVisionTransformer.forward: `pooled_output = self.post_layernorm(last_hidden_state[:, 0, :])` (vit.lnf_g / lnf_b; here
 *     of token `pool_token`), then CLIPVisionModelWithProjection.forward: `image_embeds = self.visual_projection(
 *     pooled_output)`, a bias-free Linear [proj_dim, hidden] (proj_w).  The LayerNormed row is rounded to bf16 before the
 *     projection, as the model does when it runs in bf16.
 * The attention scale (CLIPAttention: `self.scale = self.head_dim**-0.5`) is folded into the query rows as for the ViT.
 * mme_vit_forward / mme_embed then write rows of embed_dim = proj_dim, or hidden when proj_dim is 0 (see them below).
 * Validation as for the ViT loader: geometry from the same supported set, proj_dim 0 or a multiple of 64 up to 1024 (with
 * proj_w set exactly when it is not 0), act 0 or 1, non-null pre_g / pre_b; a refusal names the field, the value found and
 * the supported set, and nothing in the context changes.  The ..._as form takes the checkpoint's own element type as the
 * ViT's does.  Prepared buffers (mme_weights_read): the ViT's 6 + 18 L in their order, patch_b the zero table when NULL,
 * then pre_g [D], pre_b [D] and, with a projection, proj_w bf16 [proj_dim, D].  A later ViT load on the same context
 * returns it to the plain ViT form. */
typedef struct {
    mme_vit_weights vit;          /* patch_b may be NULL (CLIP: no bias) -> a zero table */
    const float *pre_g, *pre_b;   /* pre_layrnorm, [hidden] */
    const float* proj_w;          /* visual_projection.weight [proj_dim, hidden] or NULL */
    int32_t proj_dim;             /* 0, or a multiple of 64 up to 1024 */
    int32_t act;                  /* 0 erf-GELU, 1 QuickGELU */
} mme_clip_weights;
int mme_load_clip(mme_ctx* ctx, const mme_clip_weights* w);
int mme_load_clip_as(mme_ctx* ctx, const mme_clip_weights* w, int dtype, void* stream);
/* out[4] = kind (0 ViT, 1 CLIP, 2 SigLIP, 3 DINOv2), embed_dim (the row width the forward writes), act (0 erf-GELU, 1 QuickGELU, 2 tanh-GELU), proj_dim (0: none)
 * of the context's encoder: what the last load brought, {0, 768, 0, 0} before any. */
int mme_encoder_info(mme_ctx* ctx, int32_t out[4]);

/* ---- SigLIP ViT/16 image towers ------------------------------------------------------------------------------------------
 * Replaces `SiglipVisionModel.from_pretrained(dir)(pixel_values).pooler_output`, L2-normalised, for the towers at this
 * engine's geometry: 224 pixels, patch 16, heads of 64 (siglip-base-patch16-224 and its re-trainings).  The tower is the
 * CLIP image tower's pre-LN block sequence with these differences (transformers models/siglip/modeling_siglip.py):
 *   - SiglipVisionEmbeddings: no class token and no LayerNorm before layer 0: 196 tokens; the patch convolution HAS a bias;
 *     vit.cls_token must be NULL, vit.pos_emb is position_embedding.weight [196, hidden];
 *   - SiglipMLP: `gelu_pytorch_tanh`, 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) (act 2 of mme_encoder_info);
 *   - post_layernorm (vit.lnf_g / lnf_b) over EVERY token row, then SiglipMultiheadAttentionPoolingHead:
 *     a = MultiheadAttention(probe, h, h) with in_proj split into head.q_w | k_w | v_w [hidden, hidden] and q_b | k_b | v_b,
 *     heads of 64, out_proj = head.o_w / o_b; y = a + mlp(layernorm(a)) with head.ln2_g / ln2_b, head.fc1_*, head.fc2_* (the
 *     tower's mlp width and activation); pooler_output = y.  head.ln1_g / ln1_b are not read.
 * mme_vit_forward / mme_embed write y / max(||y||, 1e-12), rows of `hidden`; pool_token is checked (0..195) and ignored;
 * mme_set_forward_pruning has no effect (the head reads every token row); mme_preprocess writes [n * 196, 768] as for
 * patch 16.  Validation as for the ViT loader with patch_size 16 only; a refusal names the field, the value found and
 * the supported set, and nothing in the context changes.  The ..._as form takes the checkpoint's own element type.
 * Prepared buffers (mme_weights_read): the ViT's 6 + 18 L in their order (cls a zero table), then the head's ln2_g, ln2_b,
 * K | V bf16 [2 D, D], their bias [2 D], K | V with post_layernorm folded in (bf16 [2 D, D], column sums [2 D], bias' [2 D]),
 * three buffers of the query (bf16 [D, D] and f32 [D], not read; then the constant query f32 [D] =
 * (probe . W_q^T + b_q) dh^-0.5 log2 e), o_w, o_b, fc1_w, fc1_b, the fc1 fold (3), fc2_w, fc2_b: 6 + 18 L + 19.
 * A later ViT or CLIP load on the same context returns it to that form. */
typedef struct {
    mme_vit_weights vit;   /* cls_token NULL; pos_emb [196, hidden]; patch_size 16 */
    const float* probe;    /* head.probe, [hidden] */
    mme_vit_layer head;    /* ln1_g / ln1_b unused (NULL) */
} mme_siglip_weights;
int mme_load_siglip(mme_ctx* ctx, const mme_siglip_weights* w);
int mme_load_siglip_as(mme_ctx* ctx, const mme_siglip_weights* w, int dtype, void* stream);

/* ---- DINOv2 ViT/14 image towers ------------------------------------------------------------------------------------------
 * Replaces `Dinov2Model.from_pretrained(dir)(pixel_values 224 x 224).pooler_output`, L2-normalised (transformers
 * models/dinov2/modeling_dinov2.py; dinov2-small / -base / -large): the third image geometry, patch 14 at 224 pixels, 16 x 16
 * patches and a class token, 257 tokens, heads of 64.  The tower is the ViT forward (pre-LN blocks, erf-GELU, no LayerNorm
 * before layer 0, the final `layernorm` on the pooled row only) with these differences:
 *   - Dinov2Embeddings: a 14 x 14 patch convolution with bias (vit.patch_w [hidden, 588], prepared as bf16 [hidden, 640] with
 *     zero columns behind), cls_token prepended, then the position table added.  vit.pos_emb is [257, hidden] and ALWAYS host
 *     f32, under the ..._as form too: a checkpoint's [1 + g * g, hidden] table is interpolated to 16 x 16 by the caller, once,
 *     with the model's own call (checkpoint.py, interpolate_dinov2_positions).  mask_token is not read.
 *   - Dinov2Layer: x + lambda1 * attention(norm1(x)), then x + lambda2 * mlp(norm2(x)) (layer_scale1 / layer_scale2, [hidden]
 *     each: scale[l]).  LayerScale is folded at load: o_w'[n, k] = bf16(f32(lambda1[n] * o_w[n, k])), o_b'[n] =
 *     f32(lambda1[n] * o_b[n]), the same for fc2 with lambda2; the block then runs as every other tower's.
 * mme_vit_forward / mme_embed write rows of `hidden`; pool_token 0 (the default) is pooler_output, 256 the last patch token.
 * mme_preprocess writes bf16 [n * 256, 640] per crop: row PY * 16 + PX, column c * 196 + ky * 14 + kx, columns 588..639 zero.
 * Validation as for the ViT loader with patch_size 14 only (every other loader keeps refusing 14); a refusal names the
 * field, the value found and the supported set, and nothing in the context changes.  SwiGLU towers (the giant) and register
 * tokens are not run.  Prepared buffers (mme_weights_read): the ViT's 6 + 18 L in their order.  A later ViT, CLIP or SigLIP
 * load on the same context returns it to that form. */
typedef struct {
    const float* lambda1;  /* layer_scale1.lambda1, [hidden] */
    const float* lambda2;  /* layer_scale2.lambda1, [hidden] */
} mme_dinov2_scale;
typedef struct {
    mme_vit_weights vit;            /* patch_size 14; pos_emb [257, hidden], host f32 under both loaders; patch_w [hidden, 588] */
    const mme_dinov2_scale* scale;  /* [layers] */
} mme_dinov2_weights;
int mme_load_dinov2(mme_ctx* ctx, const mme_dinov2_weights* w);
int mme_load_dinov2_as(mme_ctx* ctx, const mme_dinov2_weights* w, int dtype, void* stream);

/* ---- CLIP text tower ------------------------------------------------------------------------------------------------------
 * Replaces `CLIPTextModelWithProjection.from_pretrained(dir)(input_ids).text_embeds` (or `CLIPTextModel`'s pooler_output
 * when the checkpoint has no text_projection), L2-normalised: the text side of the space a CLIP image tower embeds into
 * (transformers models/clip/modeling_clip.py, CLIPTextTransformer):
 *   - CLIPTextEmbeddings: token_embedding[ids] + position_embedding (positions 0..76);
 *   - CLIPEncoderLayer x layers, pre-LN, under the CAUSAL mask (key j reaches query i only when j <= i): layer_norm1,
 *     q / k / v, softmax(Q K^T dh^-0.5 + mask) V, out_proj + residual, layer_norm2, fc1, QuickGELU (act 1) or erf-GELU (act 0),
 *     fc2 + residual;
 *   - final_layer_norm; the row at the EOS position of each sequence (below); text_projection, a bias-free Linear
 *     [proj_dim, hidden] (proj_w, or NULL: the embedding is the LayerNormed row); x / max(||x||, 1e-12).
 * Supported geometry: 77 positions, heads of 64, hidden 512, 768 or 1024 (heads == hidden / 64: 8, 12, 16), mlp a multiple
 * of 64 up to 8192, 1..64 layers, vocab 3..65536, proj_dim 0 or a multiple of 64 up to 1024 (proj_w set exactly when it is
 * not 0), act 0 or 1, 0 <= eos_token_id < vocab, any ln_eps.  Anything else is MME_E_ARG naming the field, the value found and
 * the supported set, and nothing in the context changes.
 * The tower COEXISTS with the context's image tower: a text load touches nothing of the image side, mme_load_vit* /
 * mme_load_clip* afterwards touch nothing of the text side, a second text load frees exactly the first one's buffers.
 * mme_load_clip_text takes host f32 tensors, mme_load_clip_text_as the checkpoint's own f32 / bf16 / f16 elements (cast the
 * pointers), prepared on the device as mme_load_vit_as does; both run ONE prepare sequence and leave bit-identical buffers.
 * The LayerNorms of the layers are always folded into the QKV and fc1 GEMMs; the attention scale times log2 e is folded into
 * the query rows, as for the image towers.
 * Prepared buffers (mme_weights_read order, behind whatever the context already held; D = hidden, F = mlp, V = vocab):
 *   tok bf16 [V, D] (token_embedding, one rounding to nearest even), pos [77, D], lnf_g [D], lnf_b [D] (final_layer_norm);
 *   then 10 per layer: qkv_wf bf16 [3D, D], qkv_cs [3D], qkv_bf [3D] (the fold of layer_norm1 into Q | K | V, the Q rows
 *   times f32(dh^-0.5 log2 e)), o_w bf16 [D, D], o_b [D], fc1_wf bf16 [F, D], fc1_cs [F], fc1_bf [F] (the fold of
 *   layer_norm2), fc2_w bf16 [D, F], fc2_b [D];
 *   then, with a projection, proj_w bf16 [proj_dim, D]. */
typedef struct {
    int32_t hidden;         /* 512, 768 or 1024 */
    int32_t layers;         /* 1..64 */
    int32_t heads;          /* hidden / 64 */
    int32_t mlp;            /* multiple of 64, <= 8192 */
    int32_t vocab;          /* 3..65536 */
    int32_t max_positions;  /* 77 */
    int32_t proj_dim;       /* 0, or a multiple of 64 up to 1024 */
    int32_t act;            /* 0 erf-GELU, 1 QuickGELU */
    int32_t eos_token_id;   /* 2 selects the legacy rule of mme_text_forward */
    float ln_eps;           /* 1e-5 */
    const float* token_emb; /* [vocab, hidden] */
    const float* pos_emb;   /* [77, hidden] */
    const float* lnf_g;     /* final_layer_norm */
    const float* lnf_b;
    const float* proj_w;    /* text_projection.weight [proj_dim, hidden] or NULL */
    const mme_vit_layer* layer; /* [layers]: layer_norm1, q/k/v/out_proj, layer_norm2, fc1, fc2 */
} mme_clip_text_weights;
int mme_load_clip_text(mme_ctx* ctx, const mme_clip_text_weights* w);
int mme_load_clip_text_as(mme_ctx* ctx, const mme_clip_text_weights* w, int dtype, void* stream);
/* out[9] = loaded (0 / 1), hidden, layers, heads, mlp, vocab, proj_dim (0: none), act, eos_token_id of the context's text
 * tower; all 0 before a text load. */
int mme_text_info(mme_ctx* ctx, int32_t out[9]);
/* ids_host int32 [n, 77] (HOST) -> L2-normalised rows of text_embed_dim = proj_dim, or hidden when proj_dim is 0, to the
 * DEVICE buffers emb_f32 [n, text_embed_dim] and / or emb_bf16 (either may be NULL).  Checked on the host before any launch
 * (MME_E_ARG naming the sequence; nothing runs): every id in 0..vocab-1, and an EOS position in every sequence, found by
 * transformers' rule -- eos_token_id == 2 (legacy configurations): the first position of the sequence's largest id; else the
 * first position equal to eos_token_id, and a sequence without one is refused (transformers pools token 0 there).  Under the
 * causal mask nothing behind the EOS position reaches its row: the padding's content does not matter.
 * Works in chunks of MME_TEXT_CHUNK sequences in a workspace of its own (the image pass's buffers are not used); the rows
 * behind each EOS are computed and ignored.  MME_E_STATE before a text load; n = 0 returns MME_OK.
 * With mme_profile_enable on, the pass adds its launches to the image pass's kernel classes (token rows: preprocess; the statistics
 * passes: layernorm; GEMMs: gemm; causal attention: attention; EOS pool-LN and L2: pool): reset the profile between an image step
 * and a text call to read them apart. */
#define MME_TEXT_CHUNK 1024
#define MME_TEXT_TOKENS 77
int mme_text_forward(mme_ctx* ctx, const int32_t* ids_host, int n, float* emb_f32, uint16_t* emb_bf16, void* stream);
/* Diagnostic: ONE launch of a kernel the text tower adds, on the caller's DEVICE buffers (ids / eos_pos: HOST, validated and
 * copied), synchronous; works on a bare context.
 *   op 0 token rows        x[b*77 + t] = bf16(f32(tok[ids[b*77 + t]]) + pos[t]), b < n; tok bf16 [vocab, d], pos f32 [77, d]
 *      1 causal attention  qkv bf16 [n*77, 3*64*heads] (Q | K | V, Q pre-scaled by dh^-0.5 log2 e) -> out bf16 [n*77, 64*heads]
 *      2 EOS pool-LN       y[b] = bf16(LayerNorm(x[b*77 + eos_pos[b]]) * gamma + beta) to y bf16 [n, d] and / or the unrounded
 *                          values to y_f32 [n, d]
 * Preconditions (else MME_E_ARG, nothing launched): n >= 0; ops 0, 2: d == 512, 768 or 1024; op 1: heads == 8, 12 or 16; every
 * pointer the op uses non-null and 16-byte aligned (ids / eos_pos: non-null); op 0: 1 <= vocab <= 65536 and every id in
 * 0..vocab-1; op 2: every eos_pos in 0..76, y or y_f32. */
typedef struct mme_text_apply_args {
    const uint16_t* tok;     /* op 0 */
    const float* pos;        /* op 0 */
    const int32_t* ids_host; /* op 0: [n, 77] */
    uint16_t* x;             /* op 0: out bf16 [n*77, d]; op 2: in */
    const uint16_t* qkv;     /* op 1 */
    uint16_t* out;           /* op 1 */
    const float* gamma;      /* op 2 */
    const float* beta;
    const int32_t* eos_pos_host; /* op 2: [n] */
    uint16_t* y;             /* op 2 */
    float* y_f32;            /* op 2 */
    int32_t n, d, heads, vocab;
    float eps;
} mme_text_apply_args;
int mme_text_apply(mme_ctx* ctx, int op, const mme_text_apply_args* args, void* stream);

/* ---- SigLIP text tower ----------------------------------------------------------------------------------------------------
 * Replaces `SiglipTextModel.from_pretrained(dir)(input_ids).pooler_output`, L2-normalised: the text side of the space a SigLIP
 * image tower embeds into (transformers models/siglip/modeling_siglip.py, SiglipTextTransformer):
 *   - SiglipTextEmbeddings: token_embedding[ids] + position_embedding (positions 0..63);
 *   - SiglipEncoderLayer x layers, pre-LN, with NO mask of any kind (the model was trained on padding="max_length" without an
 *     attention_mask: pad tokens are attended), tanh-GELU (gelu_pytorch_tanh) in the MLP;
 *   - final_layer_norm; the row at position 63 of every sequence (last_hidden_state[:, -1, :], padding or not); head, a
 *     Linear [projection_size, hidden] WITH bias; x / max(||x||, 1e-12).
 * Supported geometry: max_positions 64, heads of 64, hidden 512, 768 or 1024 (heads == hidden / 64), mlp a multiple of 64 up
 * to 8192, 1..64 layers, vocab 3..262144 (SigLIP 32000, SigLIP 2 256000; every id-to-row offset is 64-bit), projection_size a
 * multiple of 64 up to 1024, 0 <= pad_token_id < vocab, any ln_eps.  Anything else (so400m's hidden 1152 / heads of 72, 77
 * positions, ...) is MME_E_ARG naming the field, the value found and the supported set, and nothing in the context changes.
 * The tower lives in the context's TEXT range: a SigLIP text load replaces a CLIP text load and vice versa, the image tower is
 * untouched, under whatever image tower the context holds.  Both loaders run the ONE prepare sequence of the text towers and
 * leave bit-identical buffers (mme_weights_read order): tok bf16 [V, D], pos [64, D], lnf_g [D], lnf_b [D]; 10 per layer as for
 * the CLIP text tower; head_w bf16 [P, D], head_b [P].
 * has_logits != 0: logit_scale / logit_bias are SiglipModel's two scalars (mme_siglip_scores); 0: the checkpoint is a bare
 * SiglipTextModel and the two fields are ignored. */
typedef struct {
    int32_t hidden;          /* 512, 768 or 1024 */
    int32_t layers;          /* 1..64 */
    int32_t heads;           /* hidden / 64 */
    int32_t mlp;             /* multiple of 64, <= 8192 */
    int32_t vocab;           /* 3..262144 */
    int32_t max_positions;   /* 64 */
    int32_t projection_size; /* multiple of 64 up to 1024 */
    int32_t pad_token_id;    /* what a caller pads short sequences with (mme_text_geometry reports it; the pass attends it) */
    int32_t has_logits;
    float ln_eps;            /* 1e-6 */
    float logit_scale;       /* the stored value: scores use exp(logit_scale) */
    float logit_bias;
    const float* token_emb;  /* [vocab, hidden] */
    const float* pos_emb;    /* [64, hidden] */
    const float* lnf_g;      /* final_layer_norm */
    const float* lnf_b;
    const float* head_w;     /* head.weight [projection_size, hidden] */
    const float* head_b;     /* head.bias [projection_size] */
    const mme_vit_layer* layer; /* [layers] */
} mme_siglip_text_weights;
int mme_load_siglip_text(mme_ctx* ctx, const mme_siglip_text_weights* w);
int mme_load_siglip_text_as(mme_ctx* ctx, const mme_siglip_text_weights* w, int dtype, void* stream);
/* out[4] = kind (0 no text tower, 1 CLIP, 2 SigLIP), tokens per sequence (77 or 64: the row length of mme_text_forward's ids),
 * projection width (0: none), pad id (SigLIP: pad_token_id; CLIP: eos_token_id, which its tokenizer pads with).
 * mme_text_info's 9 words are unchanged; under a SigLIP tower its act is 2 (tanh-GELU) and its last word is pad_token_id.
 * mme_text_forward under a SigLIP tower reads ids int32 [n, 64], checks them against the vocabulary only (there is no EOS scan)
 * and pools position 63. */
int mme_text_geometry(mme_ctx* ctx, int32_t out[4]);
/* out_f32[i] = 1 / (1 + exp(-(cos_f32[i] * exp(logit_scale) + logit_bias))), i < m * N, on DEVICE buffers (out_f32 may be
 * cos_f32): SiglipModel.forward's sigmoid of logits_per_text for a cosine block [m, N] (mme_cosine).  exp(logit_scale) is
 * formed once on the host in f32.  MME_E_STATE unless the loaded text tower is SigLIP's and brought the two scalars.
 * Enqueued on `stream`; does not synchronise. */
int mme_siglip_scores(mme_ctx* ctx, const float* cos_f32, int64_t m, int64_t N, float* out_f32, void* stream);
/* Diagnostic: ONE launch of a kernel the SigLIP text tower adds, on the caller's DEVICE buffers (ids: HOST, validated and
 * copied), synchronous; works on a bare context.
 *   op 0 token rows        x[b*64 + t] = bf16(f32(tok[ids[b*64 + t]]) + pos[t]), b < n; tok bf16 [vocab, d], pos f32 [64, d]
 *      1 attention         qkv bf16 [n*64, 3*64*heads] (Q | K | V, Q pre-scaled by dh^-0.5 log2 e) -> out bf16 [n*64, 64*heads], no
 *                          mask; only_block -1 (both query blocks of 32), 0 or 1 (that block only; the other rows of out untouched)
 *      2 last-row pool-LN  y[b] = bf16(LayerNorm(x[b*64 + 63]) * gamma + beta) to y bf16 [n, d] and / or unrounded to y_f32 [n, d]
 *      3 bias + L2         y = acc[b] + bias; emb[b] = y / max(||y||, 1e-12); acc f32 [n, p], bias f32 [p] -> emb_f32 and / or emb_bf16
 *      4 scores            scores[i] = 1 / (1 + exp(-(cos[i] * exp(logit_scale) + logit_bias))), i < count (scores may be cos)
 * Preconditions (else MME_E_ARG, nothing launched): n >= 0; ops 0, 2: d == 512, 768 or 1024; op 1: heads == 8, 12 or 16,
 * only_block in -1..1; op 3: p % 64 == 0, 64 <= p <= 1024; every pointer the op uses non-null and 16-byte aligned (ids: non-null;
 * op 4: 4-byte aligned); op 0: 1 <= vocab <= 262144 and every id in 0..vocab-1; ops 2, 3: at least one output. */
typedef struct mme_siglip_text_apply_args {
    const uint16_t* tok;     /* op 0 */
    const float* pos;        /* op 0 */
    const int32_t* ids_host; /* op 0: [n, 64] */
    uint16_t* x;             /* op 0: out bf16 [n*64, d]; op 2: in */
    const uint16_t* qkv;     /* op 1 */
    uint16_t* out;           /* op 1 */
    const float* gamma;      /* op 2 */
    const float* beta;
    uint16_t* y;             /* op 2 */
    float* y_f32;            /* op 2 */
    const float* acc;        /* op 3 */
    const float* bias;       /* op 3 */
    float* emb_f32;          /* op 3 */
    uint16_t* emb_bf16;      /* op 3 */
    const float* cos;        /* op 4 */
    float* scores;           /* op 4 */
    int64_t count;           /* op 4 */
    int32_t n, d, heads, vocab, only_block, p;
    float eps, logit_scale, logit_bias;
} mme_siglip_text_apply_args;
int mme_siglip_text_apply(mme_ctx* ctx, int op, const mme_siglip_text_apply_args* args, void* stream);

/* Diagnostic (synchronises the device): one 64-bit word per prepared weight buffer of the context, in the order the
 * loaders created them (the ViT buffers of mme_load_vit[_as], then the tile-ViT buffers of mme_load_tile_vit[_as], when
 * loaded in that order).  The word is a position-dependent checksum of the buffer's bytes -- the sum over its 32-bit words
 * of word * odd_hash(word index) mod 2^64, reduced on the device -- so two contexts hold the same prepared weights exactly
 * when their words agree, without running a forward.  Writes at most `cap` words to out_host; returns the number of
 * buffers (>= 0, call with cap = 0 to size the array) or MME_E_*. */
int mme_weights_fingerprint(mme_ctx* ctx, int cap, uint64_t* out_host);
/* odd_hash of the checksum above, for a 64-bit word index x, all arithmetic mod 2^64 (the splitmix64 finaliser, forced odd):
 *   x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *   odd_hash = (x ^ (x >> 31)) | 1.
 * The 32-bit words are little-endian; up to three bytes behind the last whole word count as one more word, zero-extended. */

/* Diagnostic (synchronises the device): copies the first min(cap_bytes, size) bytes of prepared buffer `index` to dst_host
 * and returns the buffer's size in bytes (>= 0; cap_bytes = 0 only sizes it, dst_host may be NULL then).  `index` counts in
 * the creation order mme_weights_fingerprint reports.  An index outside [0, buffers), a negative cap_bytes or a null
 * dst_host with cap_bytes > 0 returns MME_E_ARG.  tests/test_gpu_weight_prep.py compares every buffer with float64 from
 * the model's definition, and relies on this order (D = hidden, F = mlp, T = tokens; f32 unless marked bf16):
 *   ViT (mme_load_vit[_as]), 6 tables:
 *     cls [D], pos [197, D], patch_b [D], lnf_g [D], lnf_b [D], patch_w bf16 [D, 768];
 *   then 18 per layer:
 *     ln1_g [D], ln1_b [D], ln2_g [D], ln2_b [D],
 *     qkv_w bf16 [3D, D] and qkv_b [3D]: Q | K | V, the Q rows times f32(dh^-0.5 log2 e) (dh = 64; the LayerNorm-kernel mode),
 *     qkv_wf bf16 [3D, D], qkv_cs [3D], qkv_bf [3D]: the fold of ln1 (layernorm_before) into Q | K | V, Q scaled,
 *     o_w bf16 [D, D], o_b [D], fc1_w bf16 [F, D], fc1_b [F],
 *     fc1_wf bf16 [F, D], fc1_cs [F], fc1_bf [F]: the fold of ln2 (layernorm_after) into fc1,
 *     fc2_w bf16 [D, F], fc2_b [D].
 *   CLIP tower (the CLIP loaders): the ViT's 6 + 18 L buffers in that order -- patch_b all +0.0 when the tower has no patch bias,
 *     ln1 / ln2 = layer_norm1 / layer_norm2, lnf = post_layernorm -- then pre_g [D], pre_b [D] (pre_layrnorm, identical bits) and,
 *     with a projection, proj_w bf16 [proj_dim, D] (visual_projection.weight, one rounding to nearest even).
 *   Tower (mme_load_tile_vit[_as]), 11 tables:
 *     cls [1280], pos [1601, 1280] = (1 - tanh pos_gate) pos_emb, tilepos [9, 4 * 1601 * 1280] = tanh(pos_gate) tile_pos_emb,
 *     pre [9, 4 * 1280] = tanh(pre_gate) pre_emb, post [9, 4 * 1280] = tanh(post_gate) post_emb,
 *     lnpre_g, lnpre_b, lnpost_g, lnpost_b [1280], zeros [5120], patch_w bf16 [1280, 640] (columns 588..639 zero);
 *   then 9 per layer, the local stack first:
 *     qkv_wf bf16 [3840, 1280], qkv_cs [3840], qkv_bf [3840]: the fold of input_layernorm into Q | K | V, the Q rows times
 *       f32(80^-0.5 log2 e), no biases,
 *     o_w bf16 [1280, 1280] (global layers: times tanh gate_attn),
 *     fc1_wf bf16 [5120, 1280], fc1_cs [5120], fc1_bf [5120]: the fold of post_attention_layernorm into fc1,
 *     fc2_w bf16 [1280, 5120], fc2_b [1280] (global layers: both times tanh gate_ffn).
 * The fold of LayerNorm (gamma, beta) into y = W x + b:  W' = bf16(w gamma) with w = f32(scale w) on scaled rows,
 * colsum = f32(sum_k W') of the ROUNDED values, b' = f32(b + sum_k w beta_k), both sums in f64 over k ascending; every
 * factor (scale, tanh gate) is applied in f32 and rounded to f32 before anything else. */
int64_t mme_weights_read(mme_ctx* ctx, int index, int64_t cap_bytes, void* dst_host);

/* Diagnostic: ONE launch of a weight-preparation kernel (weight_prep.hip) on the caller's DEVICE buffers, then a stream
 * synchronise; works on a bare context.  `dtype` (MME_DT_*) is the element type of every source (src, w[i], b[i], gamma, beta).
 *   op 0 convert  dst[i] = src[i] (times `scale` in f32 when `scaled`), i < count, to an f32 table or, with out_bf16, to
 *                 bf16 by round-to-nearest-even (a NaN stays a quiet NaN; subnormals are not flushed).  count = 0 returns
 *                 MME_OK without a launch.
 *      1 pad      src [rows, cols] -> dst bf16 [rows, cols_padded], columns cols.. = +0.0
 *      2 fold     the LayerNorm fold described at mme_weights_read of nsrc row blocks w[i] [src_rows[i], cols] with biases
 *                 b[i] [src_rows[i]] (NULL: no bias), block i times src_scale[i] when src_scaled[i], into
 *                 wf bf16 [sum rows, cols], cs f32 [sum rows], bf f32 [sum rows]
 * Preconditions (else MME_E_ARG with a message, nothing launched): dtype 0..2; every pointer the op uses non-null (b[i]
 * excepted) and 16-byte aligned (b[i]: to its element);
 *   op 0: 0 <= count <= 2^40, count % 8 == 0;
 *   op 1: rows >= 1, cols >= 4, cols % 4 == 0, cols_padded % 4 == 0, cols_padded >= cols;
 *   op 2: nsrc in 1..3; cols % 64 == 0, 64 <= cols <= 1280; every src_rows[i] a non-zero multiple of 64, <= 2^24. */
typedef struct mme_weight_prep_apply_args {
    int32_t dtype;
    int32_t scaled, out_bf16;    /* op 0 */
    float scale;                 /* op 0 */
    const void* src;             /* ops 0, 1 */
    void* dst;                   /* ops 0, 1 */
    int64_t count;               /* op 0 */
    int32_t rows, cols_padded;   /* op 1 */
    int32_t cols;                /* ops 1, 2 */
    int32_t nsrc;                /* op 2, as everything below */
    const void* w[3];
    const void* b[3];
    int64_t src_rows[3];
    float src_scale[3];
    int32_t src_scaled[3];
    const void *gamma, *beta;
    uint16_t* wf;
    float *cs, *bf;
} mme_weight_prep_apply_args;
int mme_weight_prep_apply(mme_ctx* ctx, int op, const mme_weight_prep_apply_args* args, void* stream);

/* Pixel normalisation constants of the image processor (per channel; default CLIP).
 * Replaces the `image_mean` / `image_std` of the checkpoint's preprocessor_config. */
int mme_set_normalisation(mme_ctx* ctx, const float mean[3], const float std[3]);
/* Which form of the current constants mme_preprocess' patch emitter uses for a batch that is resized (read-only, no
 * device work; for tests and diagnostics).  *exact = 1: per channel one fma, bf16(fma(u, a[ch], b[ch])), which the host
 * verified equal to bf16 of the table entry for all 256 u when the constants were set; a / b receive that pair.
 * *exact = 0: no such pair exists near the rounded slope / offset of some channel, the emitter reads the f32 table; a / b
 * then hold nothing of meaning.  A batch of 224 x 224 crops only and mme_preprocess_tiles always read the table. */
int mme_normalisation_form(mme_ctx* ctx, int32_t* exact, float a[3], float b[3]);

/* How mme_preprocess and mme_embed make the 224 x 224 pixels of a crop (mme_preprocess_tiles ignores it).
 *   MME_RESIZE_FIT_PAD (0, what a fresh context has): the Mllama rule of one tile -- aspect-preserving fit into
 *     224 x 224, Pillow BILINEAR, zero pad right / bottom before normalisation (transformers
 *     image_processing_pil_mllama.py:246-295, 392-429, 483-541).
 *   MME_RESIZE_CLIP (1): CLIP's own rule, what CLIPImageProcessorPil does -- the short edge becomes 224 and the long
 *     edge int(224 * long / short) (transformers image_transforms.py:246-310 get_resize_output_image_size, reached from
 *     image_processing_backends.py:521-570 PilBackend.resize with size = {"shortest_edge": 224}), Pillow BICUBIC
 *     (libImaging/Resample.c, 8-bit path: a = -0.5, support 2, 22-bit coefficients, a clamp to 0..255 after each
 *     pass), then the centre crop top = (new_h - 224) / 2, left = (new_w - 224) / 2 (image_processing_backends.py:
 *     602-617 PilBackend.center_crop -> image_transforms.py:445 center_crop).  No padding ever; the uint8 window is
 *     bit-equal to Pillow's, only the window is computed.  Normalisation and the patch layout are the same as under rule 0.
 *   MME_RESIZE_SPEC (2): a rule with parameters, what a checkpoint's preprocessor_config.json asks for; made current by
 *     mme_set_resize_spec below and by nothing else: mme_set_resize_rule(2) is refused.  Rule 1 is the spec
 *     {MME_RESIZE_MODE_SHORTEST_EDGE, 224, 0, 3}, run by the same kernels.
 * A batch of 224 x 224 crops only is the identity under rules 0 and 1 and takes the same kernels.
 * Any other value is MME_E_ARG; mme_last_error names the value and the supported set.
 * The rule is a property of how the caller wants pixels made, like mme_set_normalisation: no weight load
 * (mme_load_vit*, mme_load_clip*, mme_load_tile_vit*) resets or changes it.  Crops stay limited to 1..8000 per side. */
enum { MME_RESIZE_FIT_PAD = 0, MME_RESIZE_CLIP = 1, MME_RESIZE_SPEC = 2 };
int mme_set_resize_rule(mme_ctx* ctx, int rule);
/* *rule = the current rule (read-only, no device work). */
int mme_resize_rule(mme_ctx* ctx, int32_t* rule);

/* The rule as a spec: what the Pillow backends of transformers' image processors do before rescale and normalise
 * (image_processing_backends.py PilBackend.resize -> center_crop).
 *   1. The WHOLE crop is resized with Pillow's 8-bit filter `resample` (2 BILINEAR, 3 BICUBIC; libImaging/Resample.c) to
 *      MME_RESIZE_MODE_EXACT:          height x width, the aspect not kept (ViTImageProcessor, SiglipImageProcessor: 224 x 224;
 *                                      DeiT-style processors: 256 x 256);
 *      MME_RESIZE_MODE_SHORTEST_EDGE:  the short edge becomes `height`, the long edge int(height * long / short) in f64, in
 *                                      that order of operations (BitImageProcessor as DINOv2 directories configure it: 256;
 *                                      CLIPImageProcessor: 224).  `width` must be 0.
 *      An axis whose size does not change is not filtered.
 *   2. The centre window 224 x 224 of the resized image: top = (new_h - 224) / 2, left = (new_w - 224) / 2 (the origin for an
 *      exact 224 x 224 target).  Only that window is ever computed; its uint8 pixels are bit-equal to Pillow's.
 * Supported: height (and, in exact mode, width) 224..512; resample 2 or 3.  Anything else is MME_E_ARG, mme_last_error names
 * the field, its value and the supported set, and the context keeps the rule it had.  On success mme_resize_rule reports
 * MME_RESIZE_SPEC until mme_set_resize_rule(0 | 1) leaves the spec again.  Like the two fixed rules: no weight load touches
 * it, mme_preprocess_tiles ignores it, crops stay 1..8000 per side.  A batch of 224 x 224 crops only is the identity under
 * exact 224 x 224 and under shortest edge 224, and under no other spec (shortest edge 256 resizes it to 256 x 256 and crops).
 * mme_get_resize_spec: *out = the current spec; MME_E_STATE unless a spec is the current rule.  (A C function cannot carry the
 * name of the struct's typedef, hence `get`.) */
enum { MME_RESIZE_MODE_SHORTEST_EDGE = 0, MME_RESIZE_MODE_EXACT = 1 };
typedef struct mme_resize_spec {
    int32_t mode;     /* MME_RESIZE_MODE_SHORTEST_EDGE = 0, MME_RESIZE_MODE_EXACT = 1 */
    int32_t height;   /* EXACT: height of the resized image; SHORTEST_EDGE: the edge */
    int32_t width;    /* EXACT: width of the resized image; SHORTEST_EDGE: 0 */
    int32_t resample; /* Pillow's numbers: 2 BILINEAR, 3 BICUBIC */
} mme_resize_spec;
int mme_set_resize_spec(mme_ctx* ctx, const mme_resize_spec* spec);
int mme_get_resize_spec(mme_ctx* ctx, mme_resize_spec* out);

/* Rows of the internal activation workspace = crops per encoder pass (default 4096: one pass
 * for the headline batch; 11.6 GiB of workspace at ViT-B/16; larger passes lose less to tile quantisation).
 * The workspace is 197 * crops * (12 * hidden + 2 * mlp + 8 * (1 + hidden / 64)) bytes, plus 301 056 bytes of patch
 * rows per crop in mme_embed: at 4096 crops 6.2 GB for ViT-S/16, 12.5 GB (11.6 GiB) for ViT-B/16 and 16.6 GB for
 * ViT-L/16. */
int mme_set_chunk(mme_ctx* ctx, int crops_per_pass);

/* Tuning / test knob: which MFMA GEMM tiling serves K2/K4/K6/K7/K9.  0 = by shape (default),
 * 1 = 128x128 tiles, 3 = 256x256 ping-pong kernel with a 3-deep activation ring, 4 = variant 3 with
 * 4 of a lane's 16 output stores deferred into the next tile's first K-tile (the default for large
 * problems), 6 = the 384x256 kernel (eight waves, wave tile 192x64, two K-tiles of LDS: 17 % fewer operand
 * bytes per FLOP, no deferred stores) for the epilogues it is built for (0, 1, 2, 5, 6, 8) and variant 4
 * for the others.  0 takes 6 for the (N, K) shapes on which it measured faster (QKV, fc1, fc2 of ViT-B at
 * 16 or more tiles per workgroup), else 4.  2 is accepted and means 3; 5 is accepted and means 4.  Results
 * are bit-identical across variants (same MFMA instruction, same K order per output element). */
int mme_set_gemm_variant(mme_ctx* ctx, int variant);

/* LayerNorm folding: LN1 / LN2 are folded into the QKV / fc1 GEMMs
 * (W' = W*gamma, out = rstd*(W'x - mean*colsum) + b'), so no normalised copy is written.
 *   2 (default) the per-row statistics come from partial sums the GEMM that wrote the residual
 *     stream left behind (96 bytes per row to finish; the stream is not read again);
 *   1 one statistics pass over the residual stream per LayerNorm, same canonical summation order
 *     (bit-identical embeddings to mode 2);
 *   0 separate LayerNorm kernel (A/B, tests). */
int mme_set_ln_fusion(mme_ctx* ctx, int mode);

/* K5 (attention of the ViT/16 forward, transformers modeling_vit.py:164-189).
 *   1 (default) fast form: the exponentials of a query row are taken against the maximum over its first 32 keys instead
 *     of its row maximum -- softmax is invariant to that choice, only the range differs -- which lets the scores leave
 *     the matrix pipe ready for exp2.  A row whose sum leaves [1, 2^100), or whose unnormalised output O is not finite
 *     (p v past f32's range while the sum is in range: a bf16 |v| >= 2^28), raises a per-launch guard word and the
 *     launch is redone by the exact kernel (the decision is taken on the device; the call stays asynchronous), so
 *     every finite input gets the exact algorithm's result;
 *   0 exact form only (row maximum first), as the reference computes it.
 *   2 the fast form with the guard forced for every row: every launch is redone by the exact kernel (a test of the
 *     re-run path: outputs are bit-identical to mode 0).
 * Outputs of modes 0 and 1 agree to rounding (different rounding points of the probabilities), not bit for bit.
 * The query projection carries dh^-0.5 log2(e) in every mode (folded into W_q / b_q by mme_load_vit).
 * Granularity and cost of the guard: ONE word per layer launch, so a single query row out of range re-runs that layer's
 * attention for EVERY crop of the pass (results stay correct; the launch then costs fast + exact).  The range is wide -- raw
 * scores q.k / sqrt(d) 550 apart within a row -- and seeded weights trip it only with W_q, W_k scaled x7 and more
 * (profiles/round3_fuzz_attention.txt); the redo rate on a TRAINED checkpoint is unmeasured (none is available offline):
 * mme_attention_redone says which layers of the last pass were redone, bench.py prints their count next to the headline,
 * and mode 0 is the setting for a checkpoint that trips the guard routinely.
 * The same switch governs the tile-ViT encoder's attention (mme_tile_vit_forward; attention_tiles.hip), whose fast form
 * differs: the reference point of a row starts as the maximum over its first 32 keys and is RE-CENTRED from the row sum after
 * every 128-key tile (a sum past 2^60 moves the reference by the sum's exponent: exact powers of two), so the range is left
 * only when a score jumps ~60+ log2 units above everything the row met before within one tile.  The guard is checked once per
 * row after the last key: a final sum not below 2^100 (inf / NaN included) or an O accumulator that is not finite (a jump of
 * ~67 with |v| > 1, less with a larger |v|: O overflows while re-centring keeps the sum in range) redoes that layer's launch
 * by the exact kernel (one guard word per layer, 40 for the full tower: mme_attention_redone_n). */
int mme_set_attention_mode(mme_ctx* ctx, int mode);
/* Order in which the kernels of an encoder pass walk the rows of the activations.  1 (default) zig-zag: consecutive kernels
 * walk in opposite directions, so a consumer starts on the rows its producer wrote last -- what is still in the 256 MiB
 * Infinity Cache of a 1.2-5 GB activation; 0 every kernel upwards; 2 only the attention downwards.  Tile order only: results
 * are bit-identical in every mode.  Worth 0.3-0.6 ms per step on boxes whose HBM streams at 3.9 TB/s, nothing on the others. */
int mme_set_tile_order(mme_ctx* ctx, int mode);
/* Last-layer pruning (default OFF; no reference counterpart -- the reference computes the whole last hidden state and
 * `last_pooling` then reads ONE token row of it, embedder.py:17-34).  With it on, the rows nothing reads are not computed:
 * in the last layer only the query block that holds the pooled token is attended, and its o_proj / LayerNorm / MLP run on
 * the n gathered rows instead of n x 197 (6.2 % of the forward's FLOP).  Same kernels, same per-row arithmetic: the
 * embeddings are bit-identical to the full pass.  Off by default so that the headline benchmark times the WHOLE forward
 * (bench.py reports the pruned rate separately); applies to the LayerNorm-folded modes (mme_set_ln_fusion 1 / 2). */
int mme_set_forward_pruning(mme_ctx* ctx, int on);
/* Diagnostic (synchronises the device): flags[l] != 0 when the attention launch of layer l of the LAST encoder pass
 * raised its guard and was redone by the exact kernel.  Writes min(12, layers) words (mme_vit_geometry): the whole of a
 * ViT-S or ViT-B pass; mme_attention_redone_n reads the 24 of ViT-L. */
int mme_attention_redone(mme_ctx* ctx, int32_t flags[12]);
/* As mme_attention_redone for the first `count` (1..64) layers of the last pass: the layer count of the ViT forward, the
 * tower's local + global layer count (40 in the full tower) after mme_tile_vit_forward. */
int mme_attention_redone_n(mme_ctx* ctx, int count, int32_t* flags);
/* ONE attention launch on a caller's activation, exactly as the forward makes it under the current
 * mme_set_attention_mode (0 exact; 1 fast, then the exact kernel with run_if = guard; 2 the re-run forced).  Synchronous.
 *   kind 0 (K5):       at the context's geometry (mme_vit_geometry; ViT-B/16 when nothing is loaded):
 *                      qkv_dev bf16 [n*197][3*hidden] = Q | K | V, head h at columns 64h of each part -> out_dev bf16 [n*197][hidden];
 *                      only_block -1 (every query block) or 0..6 (only queries 32b..32b+31 are computed and stored, as the
 *                      pruned last layer does); reverse 0 / 1 (the walk order of the blocks; results are bit-identical).
 *                      This is the 197-token kernel: under a patch-32 context (50 tokens) kind 0 is MME_E_ARG, and
 *                      mme_vit32_apply op 2 launches that geometry's kernel.
 *   kind 1 (tile-ViT): qkv_dev bf16 [n*6432][3840], 16 heads of 80 -> out_dev bf16 [n*6432][1280]; ntiles_host int32[n],
 *                      the tiles each image uses (1..4: the padding mask); only_block must be -1 and reverse 0.
 * Q carries dh^-0.5 log2(e) already (as after mme_load_vit / mme_load_tile_vit): the scores are base-2 logits.
 * *redone = 1 when the fast form's guard was raised and the exact kernel redid the launch (always in mode 2, never in
 * mode 0).  The launch has a guard word of its own: what mme_attention_redone reports for the last pass is unchanged. */
int mme_attention_apply(mme_ctx* ctx, int kind, const uint16_t* qkv_dev, int n, const int32_t* ntiles_host, int only_block,
                        int reverse, uint16_t* out_dev, int32_t* redone, void* stream);

/* ---- K0: cut the bounding boxes of one decoded page on the device ----------
 * Replaces DocLayoutDetector.get_region_image (doclayout_detector.py:165-194), which re-opens
 * and re-decodes the whole page PNG for every region: the page is uploaded once and every box
 * is gathered into the packed crop buffer that mme_preprocess / mme_embed read.
 *   page_dev    uint8 RGB HWC pixels of the page, [H, W, 3]
 *   boxes_host  int32[n,4] (x0, y0, x1, y1) AFTER the reference's int() truncation
 *               (doclayout_detector.py:179); crop i is (y1-y0) x (x1-x0) pixels; parts of a box
 *               outside the page read as 0, as PIL's Image.crop fills them.  A corner may be any
 *               int32, however far outside the page: sizes and byte columns are formed in 64 bits,
 *               and a box whose x1 - x0 or y1 - y0 is not in 1..8000 is MME_E_ARG, named by index
 *   pix_dev     destination buffer; offs_host int64[n] byte offset of crop i in it (the packing
 *               rule of mme_preprocess: any byte offsets, 16 bytes of slack behind the last pixel) */
int mme_crop_boxes(mme_ctx* ctx, const uint8_t* page_dev, int H, int W, const int32_t* boxes_host, int n, uint8_t* pix_dev,
                   const int64_t* offs_host, void* stream);

/* ---- the 8000-pixel cap on the device: Image.resize(..., Image.LANCZOS) of 8-bit RGB, bit for bit ----------
 * embedder.py:110-114 and :165-168 shrink an image with a side over MAX_IMAGE_HEIGHT_AND_WIDTH = 8000 with Image.LANCZOS
 * before the processor sees it.  These three entries restate Pillow's libImaging/Resample.c (8-bit path) for that filter:
 * lanczos(x) = sinc(x) sinc(x / 3) on -3 <= x < 3, support 3 * max(in / out, 1), 22-bit fixed-point coefficients rounded
 * half away from zero, horizontal pass then vertical pass, each a signed 32-bit sum from 2^21, shifted arithmetically by
 * 22 and clamped to 0..255; an axis whose size does not change is not filtered.  An image more than 100 times as high as
 * wide that gets lower is resized vertically first, as PIL/Image.py does it.  Every output byte equals Pillow's (12.2.0).
 * Accepted per axis: in 1..32768, out 1..8000, in / out <= 16 (ksize <= 97), upscaling included. */

/* The tables of one axis (embedder.py:110-114; Resample.c precompute_coeffs + normalize_coeffs_8bpc, box = whole image).
 * A pure host function without a context: it runs on a machine without a GPU and may be called from any thread (computed
 * in f64 with contraction off, calling libm's sin, the function Pillow's own object code calls).
 *   bounds  int32[out_size][2]      {xmin, n}: output coordinate xx reads source coordinates [xmin, xmin + n)
 *   coeffs  int32[out_size][ksize]  fixed-point weights of those n coordinates, zero from n on
 *   *ksize  2 * ceil(3 * max(in / out, 1)) + 1
 * With bounds and coeffs both null only *ksize is written (size the arrays with it, then call again).  A refusal's text is
 * mme_last_error(NULL). */
int mme_lanczos_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int* ksize);

/* Bytes of caller-owned device scratch that mme_lanczos_resize needs for h x w -> new_h x new_w (embedder.py:110-114;
 * Resample.c ImagingResampleInner's intermediate image): the horizontal pass's image [h][new_w * 3 rounded up to 16]
 * and both tables (the vertical-first order: three scratch images and four tables of an image at most 327 pixels wide).
 * Host function without a context, any thread. */
int mme_lanczos_workspace(int h, int w, int new_h, int new_w, size_t* bytes);

/* dst = Image.fromarray(src).resize((new_w, new_h), Image.LANCZOS) (embedder.py:110-114; Resample.c ImagingResample).
 *   src_dev   uint8 RGB HWC at ANY byte address, h rows of w pixels, src_pitch_bytes >= 3 * w apart: a box inside a
 *             larger decoded page is a valid source
 *   dst_dev   packed [new_h, new_w, 3], any byte address
 *   work_dev  work_bytes >= mme_lanczos_workspace(...) of device memory, any address, owned by the caller for the
 *             duration of the work
 * Threading: the call uses ONLY the caller's workspace and never a buffer of the context, so it cannot meet another
 * thread in the context's scratch tables; run it on the thread and stream that run mme_embed on its output (the embedder
 * and the region processor launch it from their consumer thread, on the compute stream, ordered by the events that
 * already order the pixels).  The tables are made on the host and uploaded by the call, which waits for that upload (and
 * so for the stream's earlier work); the two kernels are asynchronous on `stream`.
 * Geometry outside the accepted range is refused with the field, its value and the supported range; nothing is written. */
int mme_lanczos_resize(mme_ctx* ctx, const uint8_t* src_dev, int64_t src_pitch_bytes, int h, int w, uint8_t* dst_dev, int new_h,
                       int new_w, void* work_dev, size_t work_bytes, void* stream);

/* ---- K13: merge the detector's grid passes -- class-aware non-maximum suppression ----------
 * Replaces apply_non_max_suppression / calculate_iou (3_combine_grids.py:44-137), the O(n^2) list.index / list.pop loop
 * that turns the boxes of all grid passes of a page into the page's region list: keep the highest-scoring box left (the
 * first of equal scores), drop every remaining box of the same class whose IoU with it exceeds iou_threshold.  Many pages
 * per call, one workgroup each; float64 in the reference's operation order, so the kept set and its order are identical.
 * All pointers are HOST memory (the boxes come from JSON and the result goes back into JSON); the call returns when
 * the results are there.
 *   boxes f64[n,4] (x0,y0,x1,y1), scores f64[n], classes int32[n]; page p owns rows [page_offs[p], page_offs[p+1]),
 *   page_offs int32[pages+1] with page_offs[0] = 0, at most 32768 boxes per page
 *   keep int32[n]: for page p, keep[page_offs[p] + k] = page-local index of the k-th kept box in the reference's output
 *   order, -1 beyond keep_count[p]; keep_count int32[pages] */
int mme_nms_boxes(mme_ctx* ctx, const double* boxes, const double* scores, const int32_t* classes, const int32_t* page_offs, int pages,
                  double iou_threshold, int32_t* keep, int32_t* keep_count, void* stream);

/* ---- K1: crop -> resize -> pad -> normalise -> patchify ------------------------------
 * Replaces, per crop, `processor(images=[image])` (embedder.py:117-121; transformers
 * image_processing_pil_mllama.py:483-541 with tile 224, one tile): aspect-preserving
 * Pillow-BILINEAR fit (bit-exact incl. the per-pass uint8 rounding), zero pad right/
 * bottom BEFORE normalisation, x/255, (x-mean)/std, im2col to [196, 768] in (c,ky,kx)
 * (768 = 3 * 16 * 16, the patch row: the same at every hidden size).
 *   pix_dev     uint8 RGB HWC pixels of all crops, concatenated; the allocation must
 *               extend at least 16 bytes past the last pixel (rows are read in words)
 *   offs_host   int64[n]   byte offset of crop i inside pix_dev.  THE ALIGNMENT RULE, for mme_preprocess, mme_embed,
 *                          mme_preprocess_tiles and mme_crop_boxes alike: an offset may be ANY byte offset >= 0 and crops
 *                          may follow one another without a gap; the result is the same bit for bit wherever a crop
 *                          starts (tests/test_gpu_k1_extremes.py runs every rule at offsets 1, 2, 3, 5, 7, 9, 11, 13
 *                          and 15 mod 16).  The only requirement is the 16 bytes of allocation behind the last pixel,
 *                          above.  Starting crops at multiples of 16 is a matter of speed (the band fetch then has no
 *                          lead, and 224 x 224 crops take the 16-byte copy), not of correctness.
 *   hw_host     int32[n,2] (height, width) of crop i  (int()-truncated bbox size,
 *                          doclayout_detector.py:179)
 *   patches_dev bf16[n*196, 768]; under a patch-32 context (mme_vit_geometry: patch_size 32) bf16[n*49, 3072], the same
 *               bytes per crop: K1 writes the patch-16 matrix into an internal staging buffer and a copy kernel permutes
 *               it (four 16 x 16 patches are one 32 x 32 patch), so every pixel value is the same bit for bit */
int mme_preprocess(mme_ctx* ctx, const uint8_t* pix_dev, const int64_t* offs_host, const int32_t* hw_host,
                   int n, uint16_t* patches_dev, void* stream);

/* Mllama-faithful multi-tile preprocessing: what `processor(images=[image])`
 * (embedder.py:117-121) computes with the checkpoint's geometry -- transformers
 * image_processing_pil_mllama.py:483-541: choose the tile canvas among all grids of <= max_tiles
 * tiles (:299-355), aspect-preserving Pillow-BILINEAR fit into it (:246-295, :431-481), zero pad to
 * the canvas, x/255, (x-mean)/std (the values of mme_set_normalisation), split into tiles row-major
 * (:39-49), zero-pad the tile axis (:84-133).  Bit-exact f32.
 *   pix_dev / offs_host / hw_host   as mme_preprocess
 *   tile, max_tiles                 560 and 4 for mmE5-mllama; tile % 8 == 0
 *   out_dev            float[n, max_tiles, 3, tile, tile]  (`pixel_values`)
 *   aspect_ids_host    int32[n] or NULL: `aspect_ratio_ids` (1-based index into the supported grids, :136-164)
 *   num_tiles_host     int32[n] or NULL: tiles used; `aspect_ratio_mask` = 1 for the first num_tiles slots (:52-81)
 * Limit: the vertical pass holds the taps of one output row in 160 words of LDS.  Pillow's window of a crop of h rows
 * that becomes new_h rows is 2 * ceil(h / new_h) + 1 taps (1 when the height does not change); a batch in which some
 * crop's window exceeds 160 taps -- its height shrinks by a factor above 79, e.g. 8000 x 9 at tile 16, max_tiles 1 -- is
 * refused whole with MME_E_ARG before anything is launched (the message names the crop, its size, the window and the
 * limit; out_dev is not written).  At tile 560 with 4 tiles no crop of up to 8000 x 8000 comes near it (the canvas is
 * chosen for the largest scale, at least 1120 / 8000: a factor of 7.2 at most, 17 taps).  The
 * horizontal pass sizes its table from the crop and has no such limit.
 * Synchronises the stream once (crop tables are staged from host temporaries). */
int mme_preprocess_tiles(mme_ctx* ctx, const uint8_t* pix_dev, const int64_t* offs_host, const int32_t* hw_host, int n, int tile,
                         int max_tiles, float* out_dev, int32_t* aspect_ids_host, int32_t* num_tiles_host, void* stream);

/* ---- K2-K8: ViT forward + pool + L2 normalise -------------------------------------------
 * Replaces `model(**inputs, output_hidden_states=True)` + `last_pooling`
 * (embedder.py:124-129, :17-34).  pool_token: 0 = [CLS] (default), 196 = last token
 * (the reference's "last attended token" with an all-ones mask), any 0..196; under a patch-32 context any 0..49, and
 * patches_dev is the bf16[n*49, 3072] matrix mme_preprocess writes there.  A patch-32 pass runs its own patch embedding
 * (f32 GEMM + one row kernel), attention (exact row maximum: mme_set_attention_mode keeps its value, mme_attention_redone
 * reports zeros) and pooling kernels; every GEMM and LayerNorm form is the patch-16 pass's.
 *   emb_f32_dev  float[n, embed_dim]  L2-normalised (may be NULL)
 *   emb_bf16_dev bf16 [n, embed_dim]  same vectors rounded to bf16 (may be NULL)
 * embed_dim (mme_encoder_info) is `hidden` for a ViT and for a CLIP tower without projection, else the tower's proj_dim.
 * After a CLIP load the pass replaces CLIPVisionTransformer.forward + visual_projection (modeling_clip.py): pre_layrnorm
 * once over x (with the first LayerNorm's statistics from the same launch), QuickGELU epilogues where act is 1, and the
 * tail post_layernorm of the pooled row -> bf16 -> projection GEMM (f32 out) -> L2. */
int mme_vit_forward(mme_ctx* ctx, const uint16_t* patches_dev, int n, int pool_token,
                    float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);

/* K1 + K2-K8 in one call, chunked through the internal workspace.  This is the device
 * side of `get_image_embeddings` (embedder.py:141-226) for decoded crops. */
int mme_embed(mme_ctx* ctx, const uint8_t* pix_dev, const int64_t* offs_host, const int32_t* hw_host,
              int n, int pool_token, float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);

/* ---- patch-token rows of the last block ------------------------------------
 * mme_vit_forward / mme_embed that also return token rows: tokens_bf16_dev bf16[n, ntok, hidden], row (b, t) = the tower's
 * final LayerNorm (`layernorm` of a ViT or DINOv2, `post_layernorm` of CLIP and SigLIP) of residual row tok0 + t of crop b,
 * then x / max(||x||, 1e-12), rounded once to bf16: the bits mme_vit_forward writes to emb_bf16_dev for pool_token =
 * tok0 + t on a tower without projection.  The width is always `hidden` (CLIP's visual_projection is not applied to token
 * rows).  The pooled outputs (either may be NULL) are mme_vit_forward's / mme_embed's for pool_token, bit for bit.
 *   tok0, ntok   0 <= tok0, 1 <= ntok, tok0 + ntok <= tokens (197 / 50 / 196 / 257), else MME_E_ARG; the patch tokens are
 *                tok0 = 1 where the tower has a class token (ViT, CLIP, DINOv2), 0 for SigLIP
 * A pass that returns tokens runs the last block unpruned whatever mme_set_forward_pruning says; the setting is left as it
 * is.  Chunked as mme_vit_forward; element offsets into tokens_bf16_dev are 64-bit (65 536 crops x 196 x 768 = 9.9 G).
 * Every single-tile image tower, ln mode and GEMM variant; a tile-ViT context and a context without a load are MME_E_STATE. */
int mme_vit_tokens(mme_ctx* ctx, const uint16_t* patches_dev, int n, int pool_token, int tok0, int ntok, uint16_t* tokens_bf16_dev,
                   float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);
int mme_embed_tokens(mme_ctx* ctx, const uint8_t* pix_dev, const int64_t* offs_host, const int32_t* hw_host, int n, int pool_token,
                     int tok0, int ntok, uint16_t* tokens_bf16_dev, float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);

/* ---- mean pooling over the patches a crop covers ---------------------------
 * For a vit or dinov2 tower (class token, T = 1 + g * g tokens, g = 224 / patch), x the residual stream behind the last
 * block and y_t = LayerNorm(x[b * T + t]) * gamma + beta with the final LayerNorm's weights, in f32 (K8's arithmetic): crop b
 * has a covered grid (R, C), 1 <= R, C <= g, S_b = {1 + r * g + c : r < R, c < C}, P = R * C, and
 *     m = (sum_{t in S_b} y_t) / P                                              in f32
 *     MME_POOL_MEAN      m / max(||m||, 1e-12)                                  embed_dim = hidden
 *     MME_POOL_CLS_MEAN  v = [y_0 | m], v / max(||v||, 1e-12), one norm over    embed_dim = 2 * hidden
 *                        all 2 * hidden values (transformers' Dinov2ForImageClassification feature, L2-normalised)
 * and the bf16 output is the single rounding of the f32 output.  The summation order is a fixed function of (R, C) alone --
 * not of n, the chunk or any setting: with the covered tokens numbered j = r * C + c, partial sum p_w, w = 0..3, adds the
 * rows j = w, w + 4, w + 8, ... in ascending j starting from its first row; m = (((p_0 + p_1) + p_2) + p_3) * (1.0f / P), over
 * the partial sums that have a row.  So the grid (1, 1) gives mme_vit_forward's row for pool_token = 1 bit for bit.
 * The covered grid: under the fit-and-pad rule the resized crop sits top-left in the 224 x 224 canvas and the rest is padding
 * (half of all newspaper regions cover under a third of the patches), so R = ceil(new_h / patch), C = ceil(new_w / patch) of
 * the rule's own new_h x new_w: a patch counts when it holds at least one pixel of the crop.  Under MME_RESIZE_CLIP and every
 * MME_RESIZE_SPEC the canvas is full: (g, g).
 *
 * mme_set_pooling: MME_POOL_TOKEN (the default: one token row, pool_token, every bit as before), MME_POOL_MEAN,
 * MME_POOL_CLS_MEAN.  The mean modes need a vit or dinov2 tower loaded; with a CLIP or SigLIP tower (the projection and the
 * head pool for themselves), the tile tower or no tower they are MME_E_STATE, any other mode number MME_E_ARG.  Every image
 * tower load sets the mode back to MME_POOL_TOKEN: mme_load_vit / _clip / _siglip / _dinov2 and their _as forms, and
 * mme_load_tile_vit too -- a ViT or DINOv2 tower loaded before it stays loaded and usable, so the mean modes can be set again
 * afterwards.  A text-tower load (mme_load_clip_text, mme_load_siglip_text) replaces the text tower and nothing of the image
 * side: it leaves the mode as it is.  Under the mean modes pool_token is checked and ignored, the last block
 * runs unpruned whatever mme_set_forward_pruning says (the setting is left as it is), mme_encoder_info reports the mode's
 * embed_dim, mme_vit_forward and mme_vit_tokens pool whole grids, and mme_embed and mme_embed_tokens pool the grids of
 * mme_pool_grids.  Token rows are not affected. */
enum { MME_POOL_TOKEN = 0, MME_POOL_MEAN = 1, MME_POOL_CLS_MEAN = 2 };
int mme_set_pooling(mme_ctx* ctx, int mode);
int mme_pooling(mme_ctx* ctx, int32_t* mode);
/* The fit-and-pad covered grid of one h x w crop at `patch`: out_rc = (R, C).  A host function, no context and no GPU (errors:
 * mme_last_error(NULL)).  h, w outside 1..8000 or patch not 14, 16 or 32: MME_E_ARG. */
int mme_pool_grid(int h, int w, int patch, int32_t out_rc[2]);

/* ---- K1's plan, seen from the host ---------------------------------------------------------------------------------------
 * What mme_preprocess / mme_embed (rule kind 0: fit-and-pad; kind 1: a resize spec -- MME_RESIZE_CLIP is the spec {shortest
 * edge, 224, 0, BICUBIC}) and mme_preprocess_tiles (kind 2) decide on the host for a batch of n crops of sizes hw_host int32
 * [n, 2] (h, w): one record per crop, computed by the very functions those entry points plan with.  A host function: no
 * context and no GPU (errors: mme_last_error(NULL)).  Nothing is launched and nothing allocated on a device.
 * MME_E_ARG: a null pointer, n < 0, a kind outside 0..2, a spec mme_set_resize_spec refuses, a (tile, max_tiles)
 * mme_preprocess_tiles refuses.  A crop the entry point would refuse the BATCH for is no error here: its record says so
 * (`refused`), every other field of that record that could be computed is filled in, and planning goes on behind it as if
 * the crop were absent (it takes no table and no scratch bytes).
 * totals, if not NULL: [0] table bytes, [1] scratch bytes, [2] bands of the horizontal pass over all three classes,
 * [3] the largest kv of the batch.
 * bands_host, if not NULL: int32 [bands_cap, 4] receives the band list itself, (crop, first source row, rows, class) per band
 * in the order the entry point copies it to the device (class 0 | 1 | 2); MME_E_ARG when the batch has more than bands_cap
 * bands.  With NULL the bands are counted and not listed, which makes a record cost well under a microsecond. */
enum { MME_K1_RULE_FIT_PAD = 0, MME_K1_RULE_SPEC = 1, MME_K1_RULE_TILES = 2 };
enum {
    MME_K1_OK = 0,
    MME_K1_REFUSED_SIZE = 1,      /* h or w outside 1..8000 */
    MME_K1_REFUSED_TILE_TAPS = 2, /* tiles: the vertical window exceeds 160 taps (kv holds the window's taps) */
    MME_K1_REFUSED_H_LDS = 3,     /* the horizontal launch of this crop's class would ask for more than 160 KiB of LDS */
    MME_K1_REFUSED_V_TAPS = 4     /* fit-and-pad, spec: kv exceeds the 160 taps the vertical pass holds */
};
typedef struct mme_k1_rule {
    int32_t kind;         /* MME_K1_RULE_* */
    mme_resize_spec spec; /* kind 1 */
    int32_t tile, max_tiles; /* kind 2 */
} mme_k1_rule;
typedef struct mme_k1_record {
    int32_t new_h, new_w; /* the resized size (kind 1: of the WHOLE resized image) */
    int32_t top, left;    /* kind 1: origin of the 224 x 224 centre window in the resized image; else 0 */
    int32_t r0, nr;       /* kind 1: the source rows [r0, r0 + nr) the horizontal pass filters; else 0, h */
    int32_t th, tw;       /* kind 2: the tile grid; else 1, 1 */
    int32_t h_pass, v_pass; /* 1 when that axis is filtered (its size changes) */
    int32_t gh, kv;       /* capacities of the tables: groups of four horizontal taps; vertical taps (a multiple of 4) */
    int32_t h_class;      /* class of the horizontal pass: 0 eight-row, 1 four-row, 2 table through L1; -1: no bands */
    int32_t band_rows, n_bands; /* source rows per band and bands; 0, 0 without bands */
    int32_t h_lds;        /* dynamic LDS bytes the horizontal launch of h_class asks for if this crop is its widest; 0 without bands */
    int32_t v_lds;        /* dynamic LDS bytes of the vertical kernel if this crop's kv is the batch's largest; 0 for tiles (static LDS) */
    int32_t refused;      /* MME_K1_OK or why the entry point refuses the batch because of this crop */
    int64_t tab_off, tab_bytes; /* this crop's tables in the table buffer */
    int64_t tmp_off, tmp_bytes; /* this crop's scratch image (0 bytes without a horizontal pass under kinds 0 and 2) */
} mme_k1_record;
int mme_k1_plan(const mme_k1_rule* rule, const int32_t* hw_host, int n, mme_k1_record* out, int64_t totals[4], int32_t* bands_host,
                int64_t bands_cap);
/* The grids the pixel path of THIS context uses (its patch size and resize rule) for n crops of hw_host int32 [n, 2] (h, w):
 * grids_host int32 [n, 2].  Host only. */
int mme_pool_grids(mme_ctx* ctx, const int32_t* hw_host, int n, int32_t* grids_host);
/* mme_vit_forward under a mean mode with the covered grid of every crop: grids_host int32 [n, 2] (R, C), NULL = whole grids.
 * An entry outside 1..g is MME_E_ARG and nothing is launched; MME_POOL_TOKEN is MME_E_STATE.  The grids are copied to a
 * context-owned device buffer once per call, on `stream`. */
int mme_vit_forward_grids(mme_ctx* ctx, const uint16_t* patches_dev, int n, const int32_t* grids_host, float* emb_f32_dev,
                          uint16_t* emb_bf16_dev, void* stream);

/* f32 vectors (the reference moves embeddings as Python float lists, embedder.py:132) ->
 * L2-normalised bf16 rows, same normalisation as last_pooling (F.normalize, eps 1e-12).
 * x_dev float[rows,d] (d % 4 == 0, 16-byte aligned rows), y_dev bf16[rows,d]. */
int mme_normalise_rows(mme_ctx* ctx, const float* x_dev, int64_t rows, int d, uint16_t* y_dev, void* stream);

/* ---- K9: all-pairs cosine ---------------------------------------------------------------
 * The exact object every `collection.query` of the reference samples from
 * (weighted_region_clustering.py:79-84, region_compare.py:165-170,
 * cross_compare.py:119-123): sim[i,j] = <a_i, b_j> over L2-normalised bf16 rows,
 * f32 accumulate.  a [m,d], b [n,d] row-major, d % 64 == 0; sim f32 row-major with
 * leading dimension ld_sim >= n. */
int mme_cosine(mme_ctx* ctx, const uint16_t* a_dev, int m, const uint16_t* b_dev, int n, int d,
               float* sim_dev, int64_t ld_sim, void* stream);

/* The same block with S rounded to bf16 (round-to-nearest-even of the f32 accumulator: |error| <= 2^-9 relative, i.e.
 * <= 0.002 on a cosine): halves the bytes the compare stage writes and the next stage reads -- the [8192 x 65536] block of
 * one rank of config C4 is 1.07 GB instead of 2.15 GB.  n % 4 == 0 and ld_sim % 8 == 0 (16-byte stores).  Ranking
 * consumers that must match the f32 order (K10 / K12) keep using the f32 values; this is the output option for callers
 * that store or threshold similarities. */
int mme_cosine_bf16(mme_ctx* ctx, const uint16_t* a_dev, int m, const uint16_t* b_dev, int n, int d, uint16_t* sim_dev, int64_t ld_sim,
                    void* stream);

/* ---- K10: segmented top-k + area-weighted page reduction ---------------------------------
 * Replaces the page-pair loop of compute_image_similarity_matrix
 * (weighted_region_clustering.py:162-252).  Regions are grouped by page:
 * rows page_offs[p] .. page_offs[p+1]-1 of emb belong to page p, in collection order.
 *   emb_dev        bf16[N, d] L2-normalised region vectors
 *   area_pct_dev   double[N]  area_percentage (0-100) as stored (region_processor.py:89-93)
 *   valid_dev      uint8[N]   1 = area>0 and type in REGION_TYPES_TO_PROCESS (wrc:136)
 *   page_offs_host int32[P+1]
 *   skip_dev       uint8[P,P] 1 = pair skipped (same 20-char prefix, wrc:179-186); may be NULL
 *   max_query      10 (wrc:199), top_k 10 (wrc:210), max_dist 0.9 (wrc:223)
 *   metric         0: d = 1-cos, 1: d = 2-2cos
 *   normalise      1: divide off-diagonal by its max, diagonal = 1 (wrc:246-252)
 *   S_dev          double[P,P] */
int mme_page_similarity(mme_ctx* ctx, const uint16_t* emb_dev, int64_t N, int d, const double* area_pct_dev,
                        const uint8_t* valid_dev, const int32_t* page_offs_host, int P, const uint8_t* skip_dev,
                        int max_query, int top_k, double max_dist, int metric, int normalise, double* S_dev,
                        void* stream);

/* Multi-GPU form: compute only the page pairs whose rank in the row-major upper triangle
 * (i < j) lies in [pair_lo, pair_hi), un-normalised, every other entry of S_dev = 0.  Ranks split
 * 0..P(P-1)/2 evenly, add their S (disjoint entries: the sum is exact) and normalise once. */
int mme_page_similarity_pairs(mme_ctx* ctx, const uint16_t* emb_dev, int64_t N, int d, const double* area_pct_dev,
                              const uint8_t* valid_dev, const int32_t* page_offs_host, int P, const uint8_t* skip_dev,
                              int max_query, int top_k, double max_dist, int metric, int64_t pair_lo, int64_t pair_hi,
                              double* S_dev, void* stream);

/* ---- K11: page clustering -------------------------------------------------------------------
 * Replaces cluster_images' arithmetic (weighted_region_clustering.py:476-543): average
 * linkage + silhouette-chosen k.  S_dev double[P,P] page similarities with unit diagonal
 * (2 <= P <= 4096).
 *   n_clusters  0 = choose k in 2..min(10,P) (or ..min(3,P) when fewer than 10 entries of S
 *               exceed 0.01 off the diagonal, wrc:482-490) by silhouette, strict-> argmax
 *               from -1 (wrc:492,517); >0 = cut at that k (wrc:531-543)
 *   mode        0 = what scikit-learn >= 1.4 executes through the reference's TypeError
 *               fallback (wrc:504-509): euclidean metric over the ROWS of D = 1-S -- the
 *               path the bundled golden labels pin; 1 = D as a precomputed distance matrix
 *   labels_dev  int32[P]  sklearn label numbering (_hc_cut heap order)
 *   k_dev       int32[1]  chosen number of clusters
 *   scores_dev  double[16]: scores[k] = silhouette at k (NaN where not evaluated) */
int mme_cluster_pages(mme_ctx* ctx, const double* S_dev, int P, int n_clusters, int mode, int32_t* labels_dev,
                      int32_t* k_dev, double* scores_dev, void* stream);

/* K12 ranked neighbour lists.  Replaces the query + filter loops of
 * create_region_cross_comparison (region_compare.py:160-353) and create_cross_comparison
 * (cross_compare.py:109-235): for each query row r in [row0, row0 + nrows) of the L2-normalised
 * bf16 rows emb_dev[N, d], take the `fetch` nearest rows by cosine -- r itself included, as the
 * store's query returns it; order = stable ascending distance, i.e. similarity descending, index
 * ascending on ties -- drop r unless keep_self (region_compare.py:244), drop rows whose group id
 * equals r's (same parent page, :260; group_dev may be NULL), drop similarities outside
 * [min_sim, max_sim] (:269), keep the first top_n (:352).
 *   fetch, top_n  1..128 (the reference uses fetch = min(3 top_n, 100), top_n = 10)
 *   idx_dev   int32[nrows, top_n] row indices, -1 padded;  sim_dev  float[nrows, top_n] cosine
 * Small N: the [rows, N] cosine block is produced chunk-wise by the MFMA GEMM into an internal workspace
 * (<= 2 GiB) and consumed by a one-wave-per-row streaming top-k.  N >= 16384: fused, the block is never written
 * (mme_set_neighbour_mode).  S is never materialised either way.
 * Multi-GPU: each rank passes its own [row0, row0 + nrows) against the all-gathered emb. */
int mme_neighbours(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, int row0, int nrows,
                   int fetch, int top_n, int keep_self, float min_sim, float max_sim, int32_t* idx_dev, float* sim_dev,
                   void* stream);

/* K12 execution form: 0 = by size (default), 1 = the [rows, N] cosine block goes through the workspace in chunks,
 * 2 = fused (N >= 16384): a sampled per-row threshold, then the cosine GEMM appends only the values above it to
 * per-row candidate lists -- the block is never written; lists that overflow re-run their chunk in form 1 on the
 * device's own decision.  Results are identical. */
int mme_set_neighbour_mode(mme_ctx* ctx, int mode);

/* ---- K14: near-duplicate groups ------------------------------------------------
 * The connected components of the graph whose edges are the unordered pairs {i, j}, i < j, of rows of the L2-normalised
 * bf16 table emb_dev[N, d] with group_dev[i] != group_dev[j] (K12's group ids; NULL = every pair is admissible) and an
 * f32-accumulated cosine s_ij >= min_sim.  Against the float64 dot product s64 of the same bf16 rows, with
 * delta = 2 * d * 2^-24: s64 >= min_sim + delta is an edge, s64 < min_sim - delta is none, in between either.
 *
 * The state is caller-owned device memory behind one struct of pointers; all four calls enqueue on `stream` and never wait
 * for the device (the cosine blocks go through the K12 workspace, which grows on first use).
 *   parent      int32[N]   union-find forest, parent[i] <= i
 *   degree      int32[N]   edges at the row: an OUTPUT as it stands after the scans
 *   best        uint64[N]  most similar partner among the row's edges as a packed key (mme_duplicates_finish unpacks it)
 *   page_pairs  int32[P,P] or NULL: edges between page p and page q (page ids from page_of_dev; ids outside 0..P-1 are
 *               skipped), symmetric, within-page edges on the diagonal.  1 <= P <= 4096
 *   edges       int32[edge_cap,2] (i < j) and edge_sim float[edge_cap], or NULL with edge_cap = 0: the edge list, in
 *               arbitrary order.  A list that is full stays a valid, duplicate-free subset of the edges
 *   counters    int64[2]   [0] edges found (exact, also past edge_cap), [1] edges written to the list (<= edge_cap)
 * mme_duplicates_init   parent[i] = i, everything else zero.
 * mme_duplicates_scan   the pairs (i, j) with row0 <= i < row0 + nrows and i < j < N, accumulated into the state: scans over
 *                       disjoint row ranges that cover [0, N) are one whole run, in any order (nrows = 0 does nothing).
 *                       page_of_dev int32[N] is read only when the state has page_pairs.
 * mme_duplicates_merge  dst <- dst and src, two states over the same N rows (row shards of several GPUs, after an all-gather
 *                       of their states): the forests are united, degrees, page pairs and counters[0] add, best takes the
 *                       better partner.  Edge lists are NOT merged: dst's list and counters[1] stay as they are.
 * mme_duplicates_finish labels_dev int32[N]: the smallest row index of the row's component (a singleton labels itself);
 *                       best_idx_dev int32[N] / best_sim_dev float[N]: the most similar partner, the lower index among
 *                       bit-equal values, (-1, 0) where degree is 0; summary_dev int64[4]: edges, groups of >= 2 rows,
 *                       rows in such groups, rows of the largest such group (0 without one).  The state is not changed
 *                       and may be scanned further.
 * MME_E_ARG, with the field and the value in mme_last_error, nothing enqueued, state and context usable: d % 64 != 0, a
 * null pointer, rows outside [0, N], page_pairs with P outside 1..4096 or (scan) without page_of_dev, a NaN min_sim, a
 * negative edge_cap, merge of states of which one has page_pairs and the other has not.
 * Profiling classes: the GEMM counts as "cosine", dup_scan and merge as "neighbours", finish as "cluster". */
typedef struct mme_dup_state {
    int32_t* parent;
    int32_t* degree;
    uint64_t* best;
    int32_t* page_pairs;
    int32_t* edges;
    float* edge_sim;
    int64_t* counters;
    int64_t edge_cap;
    int32_t P;
} mme_dup_state;
int mme_duplicates_init(mme_ctx* ctx, const mme_dup_state* state, int N, void* stream);
int mme_duplicates_scan(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, const int32_t* page_of_dev,
                        float min_sim, int row0, int nrows, const mme_dup_state* state, void* stream);
int mme_duplicates_merge(mme_ctx* ctx, const mme_dup_state* dst, const mme_dup_state* src, int N, void* stream);
int mme_duplicates_finish(mme_ctx* ctx, const mme_dup_state* state, int N, int32_t* labels_dev, int32_t* best_idx_dev,
                          float* best_sim_dev, int64_t* summary_dev, void* stream);

/* ---- K18: density clusters of regions, DBSCAN over the vector table -------------
 * Adds to the reference: region_compare.py ranks regions (:160-353) and weighted_region_clustering.py clusters PAGES
 * (:476-543); neither has a region-level clustering.  K14 above is single linkage at a threshold, K15 needs k and places
 * every row; this answers "which regions belong to a recurring kind of thing, how many kinds, which to none".  The state,
 * the row-range calls and the refusals have K14's shape (mme_duplicates_* above).
 *
 * j is a NEIGHBOUR of i when i != j, group_dev[i] != group_dev[j] (NULL = every pair is admissible) and the f32-accumulated
 * cosine of the bf16 rows is >= min_sim; against the float64 dot product with delta = 2 * d * 2^-24 as K14: s64 >= min_sim
 * + delta is a neighbour, s64 < min_sim - delta is none, in between either.  count[i] = neighbours of i (self not counted).
 * i is CORE when count[i] + 1 >= min_samples (the row itself counts, as in scikit-learn).  A CLUSTER is a connected
 * component of the core rows under "neighbours"; its id is its smallest core row.  A non-core row with a core neighbour is
 * a BORDER row of the cluster of its most similar core neighbour (the lower index among bit-equal f32 values); every other
 * row is NOISE.  Integer adds, maxima of packed keys and a canonical union-find only: bit-identical from run to run.
 *
 * The state is caller-owned device memory; all calls enqueue on `stream` and never wait for the device (the cosine blocks
 * go through the K12 workspace, which grows on first use).
 *   count     int32[N]   neighbours of the row: an OUTPUT as it stands after the count calls
 *   parent    int32[N]   union-find forest over the core rows, parent[i] <= i
 *   border    uint64[N]  best core neighbour of a non-core row as a packed key (mme_density_finish unpacks it)
 *   counters  uint64[2]  [0] neighbour pairs the count calls found, [1] neighbour pairs the link calls saw
 * mme_density_init    parent[i] = i, everything else zero.
 * mme_density_count   the pairs (i, j) with row0 <= i < row0 + nrows and i < j < N, ACCUMULATED into count and counters[0]:
 *                     calls over disjoint row ranges that cover [0, N) are one count, in any order (nrows = 0 does nothing).
 * mme_density_link    the same pairs again, with the same row-range meaning (the ranges may be split differently): two core
 *                     rows are united, a core row is offered to a non-core neighbour's border key.  THE CALLER ORDERS IT
 *                     BEHIND EVERY COUNT CALL of the table (stream order on one stream suffices): a link pass that runs on
 *                     counts that are not final links rows that are not core yet wrongly, and nothing detects it.  emb_dev,
 *                     group_dev and min_sim must be those of the count calls; after link calls that cover [0, N)
 *                     counters[1] == counters[0].
 * mme_density_finish  (min_samples as in the link calls)
 *                     labels_dev int32[N]: the cluster id (its smallest core row) of a core or border row, -1 for noise;
 *                     kind_dev int32[N]: 2 core, 1 border, 0 noise;
 *                     border_idx_dev int32[N] / border_sim_dev float[N]: a border row's best core neighbour, (-1, 0) for
 *                     every other row;
 *                     summary_dev int64[6]: neighbour pairs found, clusters, core rows, border rows, noise rows, rows of
 *                     the largest cluster (0 without one).  The state is not changed.
 * At min_samples = 1 every row is core and labels equal K14's; at 2 there is no border row and the clusters are K14's groups
 * of >= 2 rows.  There is no merge entry and no multi-GPU form: counts add over row shards, but the link pass needs the
 * summed counts first.
 * MME_E_ARG, with the entry point, the field and the value in mme_last_error, nothing enqueued, state and context usable: a
 * null pointer, d % 64 != 0, a NaN min_sim, min_samples < 1, rows outside [0, N].
 * Profiling classes: the GEMM counts as "cosine", den_count and den_link as "neighbours", finish as "cluster". */
typedef struct mme_density_state {
    int32_t* count;
    int32_t* parent;
    uint64_t* border;
    uint64_t* counters;
} mme_density_state;
int mme_density_init(mme_ctx* ctx, const mme_density_state* state, int N, void* stream);
int mme_density_count(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, float min_sim, int row0, int nrows,
                      const mme_density_state* state, void* stream);
int mme_density_link(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, float min_sim, int min_samples,
                     int row0, int nrows, const mme_density_state* state, void* stream);
int mme_density_finish(mme_ctx* ctx, const mme_density_state* state, int N, int min_samples, int32_t* labels_dev, int32_t* kind_dev,
                       int32_t* border_idx_dev, float* border_sim_dev, int64_t* summary_dev, void* stream);

/* ---- K19: cluster hierarchy of regions, the mutual-reachability spanning tree ----
 * K18 above answers one threshold per run of two passes.  This computes, once, the spanning forest from whose N - 1 edges
 * the host derives the DBSCAN* clusters at EVERY threshold, HDBSCAN's threshold-free clusters and a dendrogram
 * (region_compare.cut_hierarchy / hierarchy_clusters / linkage_of), with no further GPU work.
 *
 * Input: K14's table, emb_dev bf16 [N, d], unit rows, d % 64 == 0; group_dev int32[N] or NULL with K14's meaning (a pair is
 * ADMISSIBLE when i != j and the groups differ); min_samples >= 1.
 * s(i, j) is the f32 the cosine GEMM writes for row i against row j; against the float64 dot product delta = 2 * d * 2^-24
 * as K14.  s(i, j) and s(j, i) are the same bits.
 * CORE SIMILARITY  core[i] = the (min_samples - 1)-th largest s(i, j) over the admissible j (the row itself counts towards
 *   min_samples, as in K18 and scikit-learn); +1.5 at min_samples = 1 (above every cosine); -2.0 when the row has fewer than
 *   min_samples - 1 admissible partners (below every cosine, finite).  The selection is exact for every min_samples.
 * WEIGHT  m(i, j) = min(core[i], core[j], s(i, j)) for an admissible pair.
 * THE TREE  the spanning forest of the admissible graph that is maximal under the strict total order on edges: m descending,
 *   then lo = min(i, j) ascending, then hi = max(i, j) ascending.  The order is strict, so the edge set is unique: it equals
 *   Kruskal's over the same f32 weights and is bit-identical from run to run.  (Mutual reachability ties in bulk -- every edge
 *   from a row to one of its closer neighbours weighs core[i] -- so the order is the centre of the definition.)
 *
 * The state is caller-owned device memory:
 *   core         float[N4]   N4 = N rounded up to 4, 16-byte aligned: an OUTPUT after the core calls
 *   comp         int32[N4]   16-byte aligned: the smallest row of the row's component
 *   row_key      uint64[N]   a row's best outgoing edge of the current round as a packed key
 *   parent       int32[N]    union-find forest, parent[i] <= i
 *   comp_weight  uint32[N]   per component scratch
 *   comp_edge    uint64[N]   per component scratch
 *   edges        int32[N - 1, 2]  (lo, hi), and weights float[N - 1]: the first counters[0] entries are valid; the order in
 *                which one round's edges land is not specified (the SET is; sort by the order above for one order)
 *   counters     uint64[3]   edges emitted, rounds run, components left
 * mme_hierarchy_init   one-row components, no edge, counters = {0, 0, N}.
 * mme_hierarchy_core   core[i] for row0 <= i < row0 + nrows; calls over row ranges that cover [0, N) fill core, in any order.
 * mme_hierarchy_scan   one round's scan of the rows row0 <= i < row0 + nrows against every row: row_key[i] = the best edge
 *                      from i to another component.  Calls over disjoint row ranges that cover [0, N) are one round's scan,
 *                      in any order, as mme_density_count.
 * mme_hierarchy_merge  ends the round: every component's maximal edge is emitted (once, when both ends chose it), the
 *                      components are united, comp is renewed, the keys cleared, counters updated.
 * THE CALLER ORDERS the core calls of the whole table BEFORE THE FIRST SCAN, and EVERY SCAN OF A ROUND BEFORE ITS MERGE, and
 * the merge before the next round's scans (stream order on one stream suffices): a scan on core values or components that are
 * not final chooses wrong edges, and nothing detects it.  emb_dev and group_dev must be the same in every call.  The
 * number of rounds depends on the data: repeat { scans; merge } until a round emits no edge (counters[0] stays) or
 * counters[0] == N - 1; at most ceil(log2 N) rounds emit edges.  Reading counters[0] back is the caller's one wait per round.
 * All calls enqueue on `stream` and never wait for the device (the cosine blocks go through the K12 workspace, which grows
 * on first use).  No merge of states across GPUs: a sharded form needs row_key merged by maximum per round.
 * MME_E_ARG, with the entry point, the field and the value in mme_last_error, nothing enqueued, state and context usable: a
 * null pointer, core or comp not 16-byte aligned, d % 64 != 0, min_samples < 1, rows outside [0, N].
 * Profiling classes: the GEMM counts as "cosine", hier_core and hier_scan as "neighbours", merge as "cluster". */
typedef struct mme_hierarchy_state {
    float* core;
    int32_t* comp;
    uint64_t* row_key;
    int32_t* parent;
    uint32_t* comp_weight;
    uint64_t* comp_edge;
    int32_t* edges;
    float* weights;
    uint64_t* counters;
} mme_hierarchy_state;
int mme_hierarchy_init(mme_ctx* ctx, const mme_hierarchy_state* state, int N, void* stream);
int mme_hierarchy_core(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, int min_samples, int row0, int nrows,
                       const mme_hierarchy_state* state, void* stream);
int mme_hierarchy_scan(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* group_dev, int row0, int nrows,
                       const mme_hierarchy_state* state, void* stream);
int mme_hierarchy_merge(mme_ctx* ctx, const mme_hierarchy_state* state, int N, void* stream);

/* ---- K15: spherical k-means over the vector table -------------------------------
 * Partitions the rows of the L2-normalised bf16 table emb_dev[N, d] into k clusters by cosine to a unit centroid.
 *   assign   label[i] = argmax_j s_ij, s_ij the f32-accumulated cosine of row i and centroid j (K9's GEMM); sim[i] = that
 *            value.  The order of the scores is total: a NaN is below every number, -0.0 below +0.0, among bit-equal scores
 *            the lowest j wins.  Against the float64 dot product s64 of the same bf16 rows, with delta = 2 * d * 2^-24
 *            (K14's bound): s64[label] >= max_j s64 - 2 delta and |sim - s64[label]| <= delta.
 *   update   sums[j, :] = the bf16 rows with label j, widened to f64 and added in ascending row index; counts[j] their number;
 *            for counts[j] > 0: n2 = sum_c sums[j, c]^2 (ascending c), centroids[j, c] = sums[j, c] / max(sqrt(n2), 1e-12),
 *            rounded once from f64 to bf16, nearest even.  An empty cluster keeps its centroid row; its sums are 0.  No
 *            floating-point atomics: bit-identical run to run.
 * mme_kmeans: the start centroids are the rows init_rows_host[0..k) of emb (k distinct rows), or, with NULL, what
 * state.centroids holds.  Assign against the start; then up to max_iter iterations of { update; assign; step end }, where
 * the step end counts the iteration, records the rows whose label changed, and stops the loop on the device once an
 * iteration moved no row (converged = 1; that iteration is counted).  So labels and sim always describe the returned
 * centroids; sums and counts are those of the last update (the labels the returned centroids were computed from; not
 * written with max_iter = 0, which is "assign rows to given centroids").  Everything is enqueued on `stream`; the call
 * never waits for the device (the cosine blocks and the update's scratch go through the K12 workspace, in row chunks when
 * [N, k] f32 exceeds it; init_rows_host goes up in one asynchronous copy of k int32 and may be reused on return).
 *   info  int64[4]: iterations run, rows moved by the last iteration, converged (0 / 1), clusters that were empty in the
 *         last update;  objective  f64[1]: the sum of sim in a fixed order.
 * MME_E_ARG, with the field and the value in mme_last_error, nothing enqueued, the context usable: N < 1, d % 64 != 0, k
 * outside 1..min(N, 65536), max_iter outside 0..1000, an init row outside 0..N-1 or listed twice, a null pointer.
 * Profiling classes: the GEMM counts as "cosine", everything else as "cluster". */
typedef struct mme_kmeans_state {   /* caller-owned device memory */
    uint16_t* centroids;   /* bf16 [k, d]  in: the start (unless init_rows is given); out: final */
    double*   sums;        /* [k, d] */
    int32_t*  counts;      /* [k] */
    int32_t*  labels;      /* [N] */
    float*    sim;         /* [N] cosine of each row to its centroid */
    int64_t*  info;        /* [4] iterations run, rows moved by the last iteration, converged (0/1), empty clusters */
    double*   objective;   /* [1] sum of sim */
} mme_kmeans_state;
int mme_kmeans(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, int k, const int32_t* init_rows_host, int max_iter,
               const mme_kmeans_state* state, void* stream);

/* Diagnostic: ONE step of K15 on the caller's device tensors (synchronous; works on a bare context), so that each can be
 * compared with a float64 restatement directly (tests/test_gpu_kmeans.py).
 *   op 0 ARGMAX  qsim f32 [N, ld] (ld % 4 == 0, ld >= k, 16-byte aligned), k valid columns -> labels[N], sim[N];
 *                *moved += the rows whose label differs from the labels[row] found there
 *   op 1 ASSIGN  emb bf16 [N, d] against centroids bf16 [k, d]: the GEMM into the workspace in chunks of chunk_rows rows (0 =
 *                by size), ARGMAX after each; outputs as op 0
 *   op 2 UPDATE  emb, labels (a label outside 0..k-1 belongs to no cluster) -> sums f64 [k, d], counts[k], centroids
 * run_if (optional, int32 on the device): the launches return at once unless *run_if != 0.
 * Preconditions (else MME_E_ARG with the field and the value in mme_last_error, nothing launched): op 0..2; N in 1..2^24;
 * k in 1..65536; ops 1, 2: d a multiple of 64 in 64..65536; the pointers the op uses non-null and aligned as stated. */
enum { MME_KMEANS_ARGMAX = 0, MME_KMEANS_ASSIGN = 1, MME_KMEANS_UPDATE = 2 };
typedef struct mme_kmeans_apply_args {
    const float* qsim;       /* op 0 */
    int64_t ld;              /* op 0 */
    const uint16_t* emb;     /* ops 1, 2 */
    uint16_t* centroids;     /* op 1: in; op 2: out */
    int32_t N, d, k;
    int32_t chunk_rows;      /* op 1 */
    int32_t* labels;         /* ops 0, 1: in (previous) and out; op 2: in */
    float* sim;              /* ops 0, 1 */
    int64_t* moved;          /* ops 0, 1 */
    const int32_t* run_if;
    double* sums;            /* op 2 */
    int32_t* counts;         /* op 2 */
} mme_kmeans_apply_args;
int mme_kmeans_apply(mme_ctx* ctx, int op, const mme_kmeans_apply_args* args, void* stream);

/* ---- K16: the silhouette of a partition of the vector table ----------------------
 * How well labels_dev[N] (a label outside 0..k-1 belongs to no cluster) partition the bf16 rows emb_dev[N, d] under the
 * distance 1 - x_i . x_j of the stored rows, widened exactly to f64 -- without the N x N matrix: the distances from row i to
 * the members of cluster c add up to n_c - x_i . S_c.
 *   S_c, n_c   sums and counts of K15's update on these labels (same adds, same order)
 *   g_ic = sum_t x_it S_ct,  q_i = sum_t x_it^2     in f64, each one chain of fused multiply-adds in ascending t
 *   row i with c = label[i]:  n_c == 1: s_i = 0.  Otherwise
 *       a_i = ((n_c - g_ic) - (1 - q_i)) / (n_c - 1)        the row's own distance 1 - q_i left out
 *       b_i = min over c' != c with n_c' > 0 of 1 - g_ic' / n_c'      (+inf when there is none)
 *       s_i = (b_i - a_i) / max(a_i, b_i), a NaN quotient becoming 0
 *     each formula with exactly the operations written, in that order.  A row of no cluster: s_i = NaN, not counted.
 *   sample   f64 [N] s_i; may be NULL
 *   cluster  f64 [k] the mean s_i of each cluster's rows (NaN for an empty cluster)
 *   score    f64 [1] the mean over the counted rows; NaN when fewer than two clusters have members or no row is counted
 *   info     int64 [2] rows counted, clusters with members
 *   sums     f64 [k, d], counts int32 [k]: S_c and n_c, as mme_kmeans_state's
 * The means add in a fixed order (per cluster, then over the clusters); no floating-point atomics: every output is
 * bit-identical run to run.  Everything is enqueued on `stream`; scratch comes from the K12 workspace.
 * MME_E_ARG, with the field and the value in mme_last_error, nothing enqueued, the context usable: N < 2, d % 64 != 0, k
 * outside 2..min(N, 65536), a null pointer other than sample.  Profiling class: "cluster". */
typedef struct mme_silhouette_out {   /* caller-owned device memory */
    double*  sample;    /* [N] or NULL */
    double*  cluster;   /* [k] */
    double*  score;     /* [1] */
    int64_t* info;      /* [2] rows counted, clusters with members */
    double*  sums;      /* [k, d] */
    int32_t* counts;    /* [k] */
} mme_silhouette_out;
int mme_silhouette(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* labels_dev, int k,
                   const mme_silhouette_out* out, void* stream);

/* Diagnostic: the rows kernel of K16 alone, on the caller's sums f64 [k, d] and counts int32 [k] -> sample f64 [N]
 * (enqueues; the same shape checks as mme_silhouette, every pointer non-null, emb and sums 16-byte aligned). */
int mme_silhouette_rows(mme_ctx* ctx, const uint16_t* emb_dev, int N, int d, const int32_t* labels_dev, int k,
                        const double* sums_dev, const int32_t* counts_dev, double* sample_dev, void* stream);

/* ---- K17: centre, reduce and whiten the vector table -------------------------------
 * A PCA basis fitted on the table itself: the device computes the moments and applies the projection, the host solves the
 * d x d eigenproblem in float64 (region_compare.projection_from_moments; not a hot path).
 *
 * Moments (K17a), mme_moments: emb_dev bf16 [N, d], any finite values.  With B = MME_MOMENTS_BLOCK (part of the definition,
 * not of the grid) and block b covering the rows b B .. min(N, (b + 1) B) - 1:
 *     p_b[c]    = sum_i x[i, c]             P_b[a, c] = sum_i x[i, a] x[i, c]
 *   every value widened from bf16 to f64, each sum starting from +0.0 and taking its rows in ascending i, one f64 addition per
 *   row (the product of two bf16 values is exact in f64: an fma and a multiply-then-add give the same bits);
 *     sum  = ((0 + p_0) + p_1) + ...        gram = ((0 + P_0) + P_1) + ...
 *   in ascending block order.  gram is symmetric bit for bit (the upper triangle of 64 x 64 tiles is computed and mirrored).
 *   No floating-point atomics: the result is bit-identical run to run and equal to the float64 restatement
 *   (tests/projection_reference.py).  The per-block partials go through the K12 workspace, in groups of blocks when they do
 *   not all fit; a group continues where the one before stopped, so the grouping changes no bit.
 *   sum_dev f64 [d], gram_dev f64 [d, d].
 * Projection (K17b), mme_project:  y[i, j] = sum_c (f32(x[i, c]) - mean[c]) * w[j, c],  j < m, in f32 throughout (one rounding
 *   for the difference, fused multiply-adds over c in an order the kernel chooses).  Against y64, the same expression in
 *   float64 from the same f32 mean and w:  |y - y64| <= (d + 2) 2^-24 sum_c |x[i, c] - mean[c]| |w[j, c]|.
 *   mean_dev f32 [d] and w_dev f32 [m, d] are the host's float64 mean and components rounded once to f32.  Outputs, at least one:
 *     y_f32_dev   [N, ld_y], ld_y >= m and ld_y % 4 == 0; the columns m .. ld_y - 1 are not written
 *     y_bf16_dev  [N, m], only with m % 64 == 0: the f32 rows L2-normalised exactly as mme_normalise_rows does it, bit for bit
 * Both are asynchronous on `stream` and never wait for the device (except that a workspace that has to grow is reallocated
 * behind a device synchronise, as everywhere); both work on a bare context.  Profiling class: "cluster".
 * MME_E_ARG, with the field and the value in mme_last_error, nothing enqueued, the context usable: N outside 1..2^24; d not a
 * multiple of 64, or outside 64..1024 for the moments (64..65536 for the projection); m outside 1..d; y_bf16_dev with
 * m % 64 != 0; both outputs null; y_f32_dev with ld_y < m or ld_y % 4 != 0; a null or misaligned pointer (16 bytes; 8 for
 * sum_dev and gram_dev). */
#define MME_MOMENTS_BLOCK 1024
int mme_moments(mme_ctx* ctx, const uint16_t* emb_dev, int64_t N, int d, double* sum_dev, double* gram_dev, void* stream);
int mme_project(mme_ctx* ctx, const uint16_t* emb_dev, int64_t N, int d, const float* mean_dev, const float* w_dev, int m,
                float* y_f32_dev, int64_t ld_y, uint16_t* y_bf16_dev, void* stream);

/* Diagnostic: K17a with group_blocks row blocks per workspace group (0 = what the workspace holds, 1..65535 otherwise), then a
 * stream synchronise -- so that a test can make the groups run on a small table; the bits are those of the product call. */
int mme_moments_apply(mme_ctx* ctx, const uint16_t* emb_dev, int64_t N, int d, int group_blocks, double* sum_dev, double* gram_dev,
                      void* stream);

/* Diagnostic: time one MFMA GEMM shape on random bf16 data (allocates its own operands;
 * synchronous).  epilogue 0 bias, 1 bias+GELU, 2 bias+residual, 3 patch-embed, 4 f32 out;
 * variant as mme_set_gemm_variant. */
int mme_gemm_bench(mme_ctx* ctx, int M, int N, int K, int epilogue, int variant, int iters, double* avg_ms);

/* Diagnostic: run the stamped build of the 256x256 3-deep-ring GEMM (bias epilogue) once on random data.
 * stamps_host uint64[256 workgroups][2 waves (0 and 4)][16]: s_memtime cycles summed over the K-tiles the
 * wave processed -- [0..7] the eight barrier-to-barrier intervals of a K-tile, [8] time in the counted wait,
 * [9] everything between two tiles' K loops, [10] K-tiles processed, [11] of [9]: group sync + next tile's
 * prologue issue, [12] of [9]: epilogue body (loads, math, store issue); the rest of [9] is the wait for the
 * next tile's first K-tile; [13] s_memtime cycles and [14] s_memrealtime ticks (100 MHz) of the whole kernel:
 * [13] / [14] x 100 MHz is the clock the chip held (the call runs ~0.5 s of the product kernel first). */
int mme_gemm_stamps(mme_ctx* ctx, int M, int N, int K, uint64_t* stamps_host);

/* Diagnostic: ONE launch of the MFMA GEMM  C[M,N] = A[M,K] . W[N,K]^T  with one fused epilogue on the CALLER's device
 * operands, exactly as the encoder pass makes it, then a stream synchronise (tests/test_gpu_gemm.py compares every
 * output element with float64).  Every pointer is device memory; a field the chosen epilogue does not read is ignored.
 *   epilogue  0 out = bf16(acc + bias[n])                      1 out = bf16(gelu(acc + bias[n]))
 *             2 out = bf16(acc + bias[n] + res[m,n])           (res has out's layout; res == out is the forward's in-place form)
 *             3 patch embed: row m = (crop b = m / 196, patch p = m % 196) -> out row b*197 + 1 + p,
 *               out = bf16(acc + bias[n] + pos[(1 + p) * N + n]); rows b*197 are not written.  M % 196 == 0.
 *               With ln_part set, the 256 x 256 kernel also leaves the partial sums of 8 below at those OUTPUT rows.
 *             4 outf[m * ldf + n] = acc (f32)
 *             5 out = bf16(rstd[m] * (acc - mean[m] * colsum[n]) + bias[n]), (mean, rstd) = ln_stats[2m], [2m + 1]
 *             6 as 5, then gelu
 *             8 as 2; a large-tile kernel (*ran_256 = 1) also writes, for every row of an INTERIOR row tile (256 rows;
 *               384 rows under variant 6, or under variant 0 where it takes that kernel),
 *               ln_part[(0 * N/64 + slice) * ln_part_rows + m] = sum and [(1 * N/64 + slice) * ...] = sum of squares of
 *               the ROUNDED outputs of row m over columns 64 slice .. 64 slice + 63 (f32).  Other rows carry no promise.
 *             (7, the candidate-list epilogue of mme_neighbours, is refused here: mme_select_apply op 2 launches it.)
 *   variant   as mme_set_gemm_variant (0 = by shape); K = 64 always runs the 128 x 128 kernel.  reverse_m 0 / 1: the
 *             256 x 256 kernel walks the row panels upwards / downwards (same results).
 * Preconditions (anything else returns MME_E_ARG with a message and launches nothing): M, N >= 1; K >= 64, K % 64 == 0;
 * A, W 16-byte aligned; epilogues with a bf16 output: N % 4 == 0, bias and out 16-byte aligned, ldo >= N, ldo % 8 == 0;
 * res 16-byte aligned and either == out or not overlapping it; pos 16-byte aligned with pos_rows >= 197; outf with
 * ldf >= N, 16-byte aligned when ldf % 4 == 0 (4-byte otherwise); ln_stats 8-byte, colsum 16-byte aligned; planes:
 * N % 64 == 0, ln_part_rows >= M (epilogue 8) or >= M / 196 * 197 (epilogue 3), ln_part_floats >= 2 * N/64 * ln_part_rows.
 * *ran_256 = 1 when a large-tile kernel ran (256 x 256 or 384 x 256; for epilogue 8, the planes were written), 0 for the
 * 128 x 128 one. */
typedef struct mme_gemm_apply_args {
    int32_t epilogue, variant, reverse_m;
    int32_t M, N, K;
    const uint16_t* A;      /* bf16 [M, K] */
    const uint16_t* W;      /* bf16 [N, K] */
    const float* bias;      /* [N] */
    uint16_t* out;          /* bf16, row pitch ldo elements */
    int64_t ldo;
    const uint16_t* res;    /* bf16, row pitch ldo */
    const float* pos;       /* [pos_rows, N] */
    int64_t pos_rows;
    float* outf;            /* f32, row pitch ldf elements */
    int64_t ldf;
    const float* ln_stats;  /* [M, 2] */
    const float* colsum;    /* [N] */
    float* ln_part;         /* [2][N / 64][ln_part_rows] */
    int64_t ln_part_rows;
    int64_t ln_part_floats; /* capacity of ln_part in floats */
} mme_gemm_apply_args;
int mme_gemm_apply(mme_ctx* ctx, const mme_gemm_apply_args* args, int32_t* ran_256, void* stream);

/* Diagnostic: ONE launch of a row kernel of the ViT forward on the caller's device buffers, synchronous.
 *   op 0 layernorm_rows          y[r] = bf16(LayerNorm(x[r]) * gamma + beta), r < rows; bf16 rows of d, f32 two-pass statistics
 *      1 ln_stats_rows           stats[2r], [2r + 1] = (mean, rstd) of x[r], r < rows, the same two-pass arithmetic
 *      2 ln_stats_canonical_rows the same statistics in the canonical one-pass order (gemm_epilogue.h) of rows
 *                                row0, row0 + stride, ... < row1 of x bf16 [*, d]; stats is indexed by the row itself
 *      3 ln_finish_rows          stats of rows [0, rows) from the planes part [2][d / 64][part_rows] an epilogue-8 / -3 GEMM left
 *      4 cls_rows                x[b * 197] = bf16(cls + pos[0 .. d - 1]), b < B (x bf16 [B * 197, d])
 *      5 pool_ln_l2              LayerNorm (gamma, beta) of row b * 197 + tok, then x / max(||x||, 1e-12) -> emb_f32 [B, d]
 *                                and / or emb_bf16 [B, d] (either may be NULL, not both)
 * Preconditions (else MME_E_ARG, nothing launched): the pointers the op reads or writes non-null, bf16 / f32 vectors
 * 16-byte aligned, stats 8-byte aligned; ops 0, 1, 4, 5: d == 384, d == 768 or d == 1024 (one instantiation per
 * supported width); ops 2, 3: d % 64 == 0, d <= 2048; op 2: 0 <= row0 <=
 * row1, stride >= 1; op 3: rows <= part_rows, part_floats >= 2 * d/64 * part_rows; op 5: 0 <= tok <= 196; rows, B >= 0. */
typedef struct mme_rowop_apply_args {
    uint16_t* x;            /* bf16 input rows (op 4: the rows written) */
    uint16_t* y;            /* op 0 output */
    const float* gamma;
    const float* beta;
    float* stats;           /* [*, 2] (mean, rstd) */
    const float* part;
    const float* cls;
    const float* pos;
    float* emb_f32;
    uint16_t* emb_bf16;
    int64_t rows, row0, row1, stride, part_rows, part_floats;
    int32_t d, B, tok;
    float eps;
} mme_rowop_apply_args;
int mme_rowop_apply(mme_ctx* ctx, int op, const mme_rowop_apply_args* args, void* stream);

/* Diagnostic: ONE launch of the mean-pooling kernel (pooling.hip; the definition is above mme_set_pooling) on the caller's
 * device buffers, synchronous; works on a bare context.  x bf16 [B * tokens, d]; the patch rows of crop b are first + r * g + c.
 *   op 0 mean      -> emb_f32 / emb_bf16 [B, d]
 *      1 cls+mean  -> [B, 2 d], row b * tokens the class row
 * grids: DEVICE int32 [B, 2] (R, C), or NULL for whole grids; the caller guarantees 1 <= R, C <= g (the kernel clamps).
 * Preconditions (else MME_E_ARG, nothing launched): x, gamma, beta non-null and 16-byte aligned; emb_f32 or emb_bf16 non-null,
 * both 16-byte aligned; grids 8-byte aligned; d == 384, 768 or 1024; 0 <= B <= 2^20; 1 <= g <= 16; first 0 or 1 (op 1: 1);
 * tokens == first + g * g. */
typedef struct mme_pool_apply_args {
    const uint16_t* x;
    const float* gamma;
    const float* beta;
    const int32_t* grids;
    float* emb_f32;
    uint16_t* emb_bf16;
    int32_t B, tokens, g, first, d;
    float eps;
} mme_pool_apply_args;
int mme_pool_apply(mme_ctx* ctx, int op, const mme_pool_apply_args* args, void* stream);

/* Diagnostic: ONE launch of a step of K12 (mme_neighbours) on the caller's device buffers, then a stream synchronise; works on
 * a bare context (tests/test_gpu_select.py compares every output bit with the definition above mme_neighbours).
 * The selection of ops 0 and 1, for the row with index self = row0 + r over (value, id) pairs: order by value descending, id
 * ascending; cut at `fetch`; drop id == self unless keep_self; drop id != self with group[id] == group[self] (group may be
 * NULL; it is indexed by self and by every id met); drop values outside the closed window [min_sim, max_sim]; keep the first
 * top_n into idx_out / sim_out [nrows, top_n]; pad with (-1, 0.0f).  Values compare as floats (-0 == +0, -inf is a value like
 * any other); NaN values are outside the contract.
 *   op 0 topk_rows        launch_topk_rows as mme_neighbours calls it: the pairs of row r are (qsim[r * ld + j], j), j < N.
 *                         Columns [N, ld) are not read.  run_if: a device int, or NULL; with *run_if == 0 the launch writes nothing
 *      1 topk_candidates  launch_topk_candidates: the pairs of row r are (cand_val[r * cap + k], cand_idx[r * cap + k]),
 *                         k < min(len[r], cap), ids distinct within a row; the result does not depend on their order in the list.
 *                         Slots from min(len[r], cap) on are not read
 *      2 gemm_topk        launch_gemm(EPI_TOPK, variant 3) as mme_neighbours makes it: acc = A[M, K] . W[N, K]^T (bf16 operands,
 *                         f32 accumulation); every (m, n) with acc[m, n] >= thr[m * thr_stride], n < N, takes the next slot k of row m
 *                         (cand_count[m] += 1, counted past cap as well) and, where k < cap, cand_val[m * cap + k] = acc[m, n],
 *                         cand_idx[m * cap + k] = n, in arbitrary order.  *overflow is set to 1 when some row's count exceeds cap and
 *                         is not written otherwise.  The caller zeroes cand_count[0 .. M) and *overflow first
 * Preconditions (else MME_E_ARG with the field and the value in mme_last_error, nothing launched): op 0..2; the pointers the
 * op reads or writes non-null (group and run_if excepted) and 4-byte aligned; ops 0, 1: 0 <= nrows <= 2^24, row0 >= 0, fetch
 * and top_n in 1..128; op 0: N >= 1, ld % 4 == 0, N <= ld <= 2^30, qsim 16-byte aligned; op 1: cap % 4 == 0, cap >= 4, cand_val
 * and cand_idx 16-byte aligned; op 2: 0 <= M <= 2^24, 1 <= N <= 2^20, K a multiple of 64 in 128..65536, cap >= 1,
 * thr_stride >= 1, A and W 16-byte aligned.  nrows = 0 / M = 0 launch nothing and return MME_OK. */
typedef struct mme_select_apply_args {
    const float* qsim;      /* op 0: f32 [nrows, ld] */
    const int32_t* group;   /* ops 0, 1: optional */
    int32_t* idx_out;       /* ops 0, 1: [nrows, top_n] */
    float* sim_out;         /* ops 0, 1: [nrows, top_n] */
    const int32_t* run_if;  /* op 0: optional device int */
    float* cand_val;        /* op 1: in [nrows, cap]; op 2: out [M, cap] */
    int32_t* cand_idx;      /* op 1: in [nrows, cap]; op 2: out [M, cap] */
    const int32_t* len;     /* op 1: [nrows] */
    const uint16_t* A;      /* op 2: bf16 [M, K] */
    const uint16_t* W;      /* op 2: bf16 [N, K] */
    const float* thr;       /* op 2: row m reads thr[m * thr_stride] */
    int32_t* cand_count;    /* op 2: [M] */
    int32_t* overflow;      /* op 2: one int */
    int64_t ld;             /* op 0 */
    int32_t N;              /* ops 0, 2 */
    int32_t nrows, row0, fetch, top_n, keep_self; /* ops 0, 1 */
    int32_t cap;            /* ops 1, 2 */
    int32_t M, K, thr_stride; /* op 2 */
    float min_sim, max_sim; /* ops 0, 1 */
} mme_select_apply_args;
int mme_select_apply(mme_ctx* ctx, int op, const mme_select_apply_args* args, void* stream);

/* Diagnostic: ONE launch of a kernel the CLIP tower adds, on the caller's device buffers, synchronous; works on a bare context.
 *   op 0 the GEMM of `gemm` with out = bf16(quick_gelu(acc + bias[n])), quick_gelu(x) = x * sigmoid(1.702 x)
 *        (activations.py QuickGELUActivation); gemm->epilogue is not read; operands and preconditions as epilogue 1 above
 *      1 the same with the folded LayerNorm first: quick_gelu(rstd[m] * (acc - mean[m] * colsum[n]) + bias[n]), as epilogue 6
 *      2 pre_ln_rows   x[r] = bf16(LayerNorm(x[r]) * gamma + beta) IN PLACE, r < rows (rows of d; layernorm_rows' arithmetic),
 *                      and stats[2r], [2r + 1] = (mean, rstd) of the ROUNDED row in the canonical order: the bits op 2 of
 *                      the row-kernel diagnostic above finds in x afterwards
 *      3 pool_ln_rows  y[b] = bf16(LayerNorm(x[b * 197 + tok]) * gamma + beta), b < B, y bf16 [B, d]
 *      4 l2_rows       xf f32 [rows, p] -> xf / max(||xf||, 1e-12) to y_f32 [rows, p] and / or y_bf16 (not both NULL)
 * Preconditions (else MME_E_ARG, nothing launched): op 0..4; ops 0, 1: `gemm` non-null and what the GEMM diagnostic asks of
 * epilogues 1 / 6; ops 2, 3: d == 384, 768 or 1024, x / gamma / beta non-null and 16-byte aligned; op 2: stats non-null and
 * 8-byte aligned, rows >= 0; op 3: y non-null and 16-byte aligned, B >= 0, 0 <= tok <= 196; op 4: p % 64 == 0, 64 <= p <= 1024, xf and the outputs 16-byte aligned. */
typedef struct mme_clip_apply_args {
    const mme_gemm_apply_args* gemm; /* ops 0, 1 */
    uint16_t* x;            /* ops 2 (in place), 3: bf16 rows of d */
    const float* gamma;
    const float* beta;
    float* stats;           /* op 2: [rows, 2] */
    uint16_t* y;            /* op 3: bf16 [B, d] */
    const float* xf;        /* op 4 */
    float* y_f32;
    uint16_t* y_bf16;
    int64_t rows;
    int32_t d, B, tok, p;
    float eps;
    int32_t* ran_256;       /* ops 0, 1, optional: set to 1 when the 256 x 256 kernel ran, 0 for the 128 x 128 one */
} mme_clip_apply_args;
int mme_clip_apply(mme_ctx* ctx, int op, const mme_clip_apply_args* args, void* stream);

/* Diagnostic: ONE launch of a kernel a patch-32 tower (ViT/32 @224: 49 patches of 32 x 32, 50 tokens) adds, on the caller's
 * device buffers, synchronous; works on a bare context.  n = crops (B of the pool forms).
 *   op 0 retile_patches_p32  src bf16 [n * 196, 768] (what K1 writes) -> dst bf16 [n * 49, 3072], conv order (c, ky, kx):
 *                            dst[b * 49 + PY * 7 + PX][c * 1024 + KY * 32 + KX] =
 *                            src[b * 196 + (2 PY + KY / 16) * 14 + 2 PX + KX / 16][c * 256 + (KY % 16) * 16 + KX % 16]
 *      1 embed_rows_t50      acc f32 [n * 49, d] -> x bf16 [n * 50, d]: x[b * 50 + 1 + p] = bf16((acc[b * 49 + p] + bias) + pos[1 + p]),
 *                            x[b * 50] = bf16(cls + pos[0]); pos f32 [50, d], f32 adds in that order
 *      2 attn_short<50>      qkv bf16 [n * 50, 3 * 64 * heads] (Q | K | V, Q pre-scaled by dh^-0.5 log2 e) -> out bf16 [n * 50, 64 * heads];
 *                            exact row maximum under every attention mode; only_block 0 / 1: rows 0..31 / 32..49 of every crop only
 *      3 pool_ln_rows (50)   y[b] = bf16(LayerNorm(x[b * 50 + tok]) * gamma + beta), y bf16 [n, d]
 *      4 pool_ln_l2 (50)     the same row, LayerNorm then x / max(||x||, 1e-12), to emb_f32 and / or emb_bf16 [n, d]
 * Preconditions (else MME_E_ARG, nothing launched): op 0..4; 0 <= n <= 2^20; every tensor an op reads or writes non-null
 * and 16-byte aligned (op 4: one of the two outputs may be NULL); op 0: src != dst; ops 1, 3, 4: d == 384, 768 or 1024;
 * op 2: heads == 6, 12 or 16, only_block in -1..1; ops 3, 4: 0 <= tok <= 49. */
typedef struct mme_vit32_apply_args {
    const uint16_t* src;    /* op 0 */
    uint16_t* dst;
    const float* acc;       /* op 1 */
    const float* bias;
    const float* pos;
    const float* cls;
    uint16_t* x;            /* op 1: out; ops 3, 4: in, bf16 rows of d */
    const uint16_t* qkv;    /* op 2 */
    uint16_t* out;
    const float* gamma;     /* ops 3, 4 */
    const float* beta;
    uint16_t* y;            /* op 3 */
    float* emb_f32;         /* op 4 */
    uint16_t* emb_bf16;
    int32_t n, d, heads, only_block, tok;
    float eps;
} mme_vit32_apply_args;
int mme_vit32_apply(mme_ctx* ctx, int op, const mme_vit32_apply_args* args, void* stream);

/* Diagnostic: ONE launch of a kernel a SigLIP tower adds, on the caller's device buffers, synchronous; works on a bare context.
 * (The 196-token attention kernel is launched by mme_attention_apply kind 0 under a SigLIP context.)  n = crops.
 *   op 0 the GEMM of `gemm` with out = bf16(gelu_tanh(acc + bias[n])), gelu_tanh(x) = 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)));
 *        gemm->epilogue is not read; operands and preconditions as epilogue 1 of mme_gemm_apply
 *      1 the same with the folded LayerNorm first: gelu_tanh(rstd[m] * (acc - mean[m] * colsum[n]) + bias[n]), as epilogue 6
 *      2 embed_rows_t196  acc f32 [n * 196, d] -> x bf16 [n * 196, d]: x[b * 196 + p] = bf16((acc[b * 196 + p] + bias) + pos[p]),
 *                         pos f32 [196, d], f32 adds in that order
 *      3 map_pool         kv bf16 [n * 196, 2 * 64 * heads] (K | V), q f32 [64 * heads] (in log2 units: dh^-0.5 log2 e applied) ->
 *                         out bf16 [n, 64 * heads]: per (crop, head) softmax_j(q_h . k_j) . v, exact maximum, f32 sums, one rounding
 *      4 l2_rows_bf16     x bf16 [n, d] -> x / max(||x||, 1e-12) to emb_f32 and / or emb_bf16 [n, d]
 * Preconditions (else MME_E_ARG, nothing launched): op 0..4; ops 0, 1: `gemm` non-null and what the GEMM diagnostic asks of
 * epilogues 1 / 6; ops 2..4: 0 <= n <= 2^20, every tensor the op reads or writes non-null and 16-byte aligned (op 4: one of
 * the two outputs may be NULL); ops 2, 4: d == 384, 768 or 1024; op 3: heads == 6, 12 or 16. */
typedef struct mme_siglip_apply_args {
    const mme_gemm_apply_args* gemm; /* ops 0, 1 */
    int32_t* ran_256;       /* ops 0, 1, optional: set to 1 when the 256 x 256 kernel ran, 0 for the 128 x 128 one */
    const float* acc;       /* op 2 */
    const float* bias;
    const float* pos;
    uint16_t* x;            /* op 2: out; op 4: in */
    const uint16_t* kv;     /* op 3 */
    const float* q;
    uint16_t* out;
    float* emb_f32;         /* op 4 */
    uint16_t* emb_bf16;
    int32_t n, d, heads;
} mme_siglip_apply_args;
int mme_siglip_apply(mme_ctx* ctx, int op, const mme_siglip_apply_args* args, void* stream);

/* Diagnostic: ONE launch of a kernel a DINOv2 tower (ViT/14 @224: 256 patches of 14 x 14, 257 tokens) adds, on the caller's
 * device buffers, synchronous; works on a bare context.  n = crops.
 *   op 0 retile_patches_p14  src bf16 [n * 196, 768] (what K1 writes) -> dst bf16 [n * 256, 640], conv order (c, ky, kx):
 *                            dst[b * 256 + PY * 16 + PX][c * 196 + ky * 14 + kx] = src[b * 196 + (y / 16) * 14 + x / 16][c * 256 + (y % 16) * 16 + x % 16]
 *                            with (y, x) = (14 PY + ky, 14 PX + kx); columns 588..639 are written as zero
 *      1 embed_rows_t257     acc f32 [n * 256, d] -> x bf16 [n * 257, d]: x[b * 257 + 1 + p] = bf16((acc[b * 256 + p] + bias) + pos[1 + p]),
 *                            x[b * 257] = bf16(cls + pos[0]); pos f32 [257, d], f32 adds in that order
 *      2 attn_mid            qkv bf16 [n * 257, 3 * 64 * heads] (Q | K | V, Q pre-scaled by dh^-0.5 log2 e) -> out bf16 [n * 257, 64 * heads];
 *                            exact row maximum under every attention mode; only_block 0..8: rows 32 b .. 32 b + 31 of every crop only
 *      3 pool_ln_l2 (257)    LayerNorm of row b * 257 + tok, then x / max(||x||, 1e-12), to emb_f32 and / or emb_bf16 [n, d]
 *      4 rowscale            w [rows, cols] and factor [rows] of `dtype` -> prepared bf16 [rows, cols] = bf16_rne(f32(factor[r] * w[r, k]))
 *      5 mul                 w [rows] and factor [rows] of `dtype` -> prepared f32 [rows] = f32(factor[r] * w[r])
 * Preconditions (else MME_E_ARG, nothing launched): op 0..5; ops 0..3: 0 <= n <= 2^20, every tensor the op reads or writes
 * non-null and 16-byte aligned (op 3: one of the two outputs may be NULL); op 0: src != dst; ops 1, 3: d == 384, 768 or 1024;
 * op 2: heads == 6, 12 or 16, only_block in -1..8; op 3: 0 <= tok <= 256; ops 4, 5: dtype an MME_DT_*, 1 <= rows <= 2^24, w / factor /
 * prepared non-null; op 4: w and prepared 16-byte aligned, cols a multiple of 8 in 8..65536. */
typedef struct mme_dinov2_apply_args {
    const uint16_t* src;    /* op 0 */
    uint16_t* dst;
    const float* acc;       /* op 1 */
    const float* bias;
    const float* pos;
    const float* cls;
    uint16_t* x;            /* op 1: out; op 3: in, bf16 rows of d */
    const uint16_t* qkv;    /* op 2 */
    uint16_t* out;
    const float* gamma;     /* op 3 */
    const float* beta;
    float* emb_f32;
    uint16_t* emb_bf16;
    const void* w;          /* ops 4, 5 */
    const void* factor;
    void* prepared;
    int64_t rows, cols;
    int32_t n, d, heads, only_block, tok, dtype;
    float eps;
} mme_dinov2_apply_args;
int mme_dinov2_apply(mme_ctx* ctx, int op, const mme_dinov2_apply_args* args, void* stream);

/* Diagnostic: time the attention kernel (K5) on B crops of random activations (avg_ms over iters launches), then run
 * its stamped build once, both in the form mme_set_attention_mode selects (0: the exact kernel; 1 / 2: the fast one,
 * timed with its guarded exact re-run).  stamps_host uint64[B workgroups][8 waves][8]: s_memtime cycles summed over the head
 * iterations of the wave (the context's head count: 12 for ViT-B/16) -- [0] wait for its own requests, [1] workgroup barrier, [2] issue of the next head's
 * requests (K/V LDS-DMA on wave 7, Q prefetch on the others), [3] S^T = K.Q^T, [4] softmax, [5] O^T = V^T.P^T,
 * [6] hand-over + output stores; [7] heads processed.  Wave 7 (staging only) carries in [5] / [6] the s_memtime cycles and
 * s_memrealtime ticks (100 MHz) of the whole workgroup: [5] / [6] x 100 MHz = the clock the chip held. */
int mme_attention_stamps(mme_ctx* ctx, int B, int iters, double* avg_ms, uint64_t* stamps_host);

/* ---- tile-ViT encoder option: the reference encoder's own vision-tower geometry -------------------
 * Replaces the vision side of `MllamaForConditionalGeneration.from_pretrained(...)` / `model(**inputs)`
 * (deprecated_package/embedder.py:75-79,117-126): transformers `MllamaVisionModel` at the checkpoint's configuration
 * (config.py:58; configuration_mllama.py:61-82 at image_size 560) -- <= 4 tiles of 560 x 560, patch 14, 1 + 1600 tokens
 * per tile padded to 1608, ONE sequence of 6432 tokens per image, 1280-d, 16 heads of 80, MLP 5120, `layers` local +
 * `global_layers` tanh-gated layers (32 + 8), the states after `intermediate[]` local layers (3, 7, 15, 23, 30)
 * concatenated behind the final state -> 1280 * (1 + n_intermediate) = 7680 features per token.  Geometry is fixed
 * at compile time; the layer counts are free (tests run shallow stacks against the CPU oracle).
 * Host f32 tensors in the Hugging Face state-dict layout: Linear weights [out, in]; patch_w [1280, 3*14*14] in
 * (c, ky, kx) order; pos_emb [1601, 1280]; tile_pos_emb [9, 4*1601*1280]; pre_emb / post_emb [9, 4*1280].
 * Values are rounded to bf16 on upload; the tanh gates are folded into the tables / weights they scale. */
enum { MME_TILE_SAVE_AFTER_LAYER = 0, MME_TILE_SAVE_BEFORE_LAYER = 1 };

typedef struct {
    const float *ln1_g, *ln1_b;           /* input_layernorm */
    const float *q_w, *k_w, *v_w, *o_w;   /* no biases */
    const float *ln2_g, *ln2_b;           /* post_attention_layernorm */
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    float gate_attn, gate_ffn;            /* raw parameters; tanh is applied by the library */
    int32_t gated;                        /* 1 for the global stack */
} mme_tile_layer;

typedef struct {
    int32_t image_size;  /* 560 */
    int32_t patch_size;  /* 14 */
    int32_t hidden;      /* 1280 */
    int32_t heads;       /* 16 */
    int32_t mlp;         /* 5120 */
    int32_t max_tiles;   /* 4 */
    int32_t aspect_ratios; /* 9 = max_aspect_ratio_id + 1 */
    int32_t layers, global_layers;
    int32_t n_intermediate;
    int32_t intermediate[8];
    /* Which state `intermediate[k] = i` names.  MME_TILE_SAVE_AFTER_LAYER: the OUTPUT of local layer i -- what
     * transformers 5.15's MllamaVisionEncoder collects (`encoder_states` is appended after each layer; the version the
     * oracle and tests/golden/tile_vit_cases.npz are pinned to).  MME_TILE_SAVE_BEFORE_LAYER: the state ENTERING local
     * layer i (= the output of layer i - 1; i = 0: the embeddings after layernorm_pre) -- the convention of encoders that
     * record the state before running a layer (reported for the first Mllama releases around transformers 4.45 and the
     * original model code; NOT verifiable offline, "parity unpinned": tested against the oracle's own restatement only).
     * A binder picks the convention of the transformers version its checkpoint's features were produced with. */
    int32_t intermediate_save_point;
    float norm_eps;      /* 1e-5 (the encoder layers; layernorm_pre / _post use torch's default 1e-5 too) */
    float pos_gate, pre_gate, post_gate;
    const float* class_embedding;
    const float* patch_w;
    const float* pos_emb;
    const float* tile_pos_emb;
    const float* pre_emb;
    const float* post_emb;
    const float *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b;
    const mme_tile_layer* layer; /* [layers + global_layers], local stack first */
} mme_tile_vit_weights;

int mme_load_tile_vit(mme_ctx* ctx, const mme_tile_vit_weights* w);
/* As mme_load_vit_as: every tensor pointer of `w` and of its layers points at host elements of `dtype` (MME_DT_*), prepared
 * on the device bit-identically to mme_load_tile_vit.  The scalar gates stay `float` by value; tanh stays on the host. */
int mme_load_tile_vit_as(mme_ctx* ctx, const mme_tile_vit_weights* w, int dtype, void* stream);

/* pixel_values_dev f32 [n, 4, 3, 560, 560] (what mme_preprocess_tiles writes), aspect_ids_host / num_tiles_host int32[n]
 * (its other two outputs).  Any of the three outputs may be NULL:
 *   hidden_dev    f32 [n, 4, 1601, F]   `last_hidden_state` of the vision model (padding tiles included, as the model returns them)
 *   emb_f32_dev   f32 [n, F], emb_bf16_dev bf16 [n, F]   the class token of tile 0, L2-normalised: the crop's vector for
 *                 the compare stage (last_pooling's rule -- one token row, F.normalize -- embedder.py:17-34).
 * F = 1280 * (1 + n_intermediate).  Images are processed mme_set_chunk (<= 64) at a time. */
int mme_tile_vit_forward(mme_ctx* ctx, const float* pixel_values_dev, const int32_t* aspect_ids_host, const int32_t* num_tiles_host, int n,
                         float* hidden_dev, float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);

/* Diagnostic: ONE launch of a row kernel of the tile-ViT forward (tilevit.hip) on the caller's device buffers, synchronous;
 * works on a bare context, no weights loaded (tests/test_gpu_tile_rows.py compares every output element with float64).
 * Rows are 1280 wide; a padded sequence row is r = (image * 4 + tile) * 1608 + tok, an output row (image * 4 + tile) * 1601 + tok.
 *   op 0 tile_patchify  pv f32 [tiles, 3, 560, 560] -> patches bf16 [npatch, 640]: patch p = (tile, py, px) of the 40 x 40 grid,
 *                       element (c, ky, kx), columns 588..639 zero
 *      1 tile_assemble  x[r] = bf16(LayerNorm(v) * gamma + beta), r < rows, with v = cls + pos[0] + tilepos[a][tile][0] for tok 0,
 *                       v = pemb[(image * 4 + tile) * 1600 + tok - 1] + pre[a][tile] + pos[tok] + tilepos[a][tile][tok] for
 *                       1 <= tok <= 1600, a = aid[image]; rows with tok >= 1601 are zero.  pre [aspect_rows, 4, 1280],
 *                       pos [1601, 1280], tilepos [aspect_rows, 4, 1601, 1280] f32
 *      2 tile_ln_post   x[r] <- bf16(LayerNorm(x[r]) * gamma + beta + post[aid[image]][tile]), r < rows, in place, every row
 *      3 tile_output    hidden f32 [out_rows, 1280 * (1 + ni)]: features [0, 1280) = x of the source row (the 7 padding rows of
 *                       a tile are skipped), feature 1280 + d * ni + k = inter[k * inter_stride + source row * 1280 + d]
 *      4 tile_pool      row (image * 4) * 1608 of x and of the ni states, all 1280 * (1 + ni) features in that order, divided by
 *                       max(its L2 norm, 1e-12) -> emb_f32 [n, F] and / or emb_bf16 [n, F] (either may be NULL, not both)
 * `aid` is DEVICE int32, one entry per image the rows touch; the entry copies it back and refuses a value outside
 * [0, aspect_rows), aspect_rows (1..9) being the rows of the caller's pre / post / tilepos tables.
 * Preconditions (else MME_E_ARG with a message, nothing launched): the pointers the op reads or writes non-null and 16-byte
 * aligned (aid: 4-byte); inter NULL exactly when ni == 0; ni in 0..8; with ni > 1, inter_stride >= the elements one state
 * needs ((last source row + 1) * 1280) and <= 2^40; npatch, rows, out_rows, n >= 0 (a count of 0 returns MME_OK without a
 * launch) and <= 2^31 - 1. */
typedef struct mme_tile_rowop_apply_args {
    const float* pv;          /* op 0 */
    uint16_t* patches;        /* op 0 output */
    const uint16_t* pemb;     /* op 1: bf16 [*, 1280] patch embeddings */
    const float *cls, *pre, *pos, *tilepos;  /* op 1 */
    const float *gamma, *beta;               /* ops 1, 2 */
    const float* post;        /* op 2: [aspect_rows, 4, 1280] */
    const int32_t* aid;       /* ops 1, 2 */
    uint16_t* x;              /* op 1 output, op 2 in place, ops 3, 4 input */
    const uint16_t* inter;    /* ops 3, 4: ni states of inter_stride elements */
    float* hidden;            /* op 3 output */
    float* emb_f32;           /* op 4 outputs */
    uint16_t* emb_bf16;
    int64_t npatch, rows, out_rows, inter_stride;
    int32_t n, ni, aspect_rows;
    float eps;
} mme_tile_rowop_apply_args;
int mme_tile_rowop_apply(mme_ctx* ctx, int op, const mme_tile_rowop_apply_args* args, void* stream);

/* ---- Mllama language tower with cross-attention ---------------------------
 * Replaces the language side of `MllamaForConditionalGeneration.from_pretrained(...)` / `model(**inputs)` and `last_pooling`
 * (deprecated_package/embedder.py:17-34, 102-129, 228-254): transformers `multi_modal_projector` + `MllamaTextModel`
 * (models/mllama/modeling_mllama.py) -- embed_tokens, rotary positions 0..S-1, self-attention layers (RMSNorm, bias-free
 * q/k/v, rotate_half RoPE, causal GQA attention, o_proj, RMSNorm, down(silu(gate) * up)) and, at the indices of
 * cross_attention_layers, cross-attention layers (q_norm / k_norm per head, no RoPE, not causal, tanh gates, the per-row tile
 * mask of _prepare_cross_attention_mask), the final norm -- then the row at len - 1, L2-normalised.  Without vision rows
 * the cross layers are skipped entirely (the text-only path of get_text_embeddings).
 *
 * Supported geometry (else MME_E_ARG naming the field, the value found and the supported set; nothing in the context
 * changes): head_dim 128, hidden = heads * 128, heads <= 64, heads / kv_heads in {1, 2, 4, 8}; intermediate % 64 == 0 and
 * <= 16384; 1..64 layers, cross layer indices strictly increasing (an index at or beyond `layers` is ignored); vocab + 8 <=
 * 2^18 rows of embed_tokens; vision_dim % 64 == 0 and <= 8192; hidden_act 0 (silu); rope_type 0 ("default") or 1 ("llama3");
 * image_token_id in 0..vocab + 7.  Sequences of 1..128 tokens.
 *
 * Every tensor is row-major f32 (mme_load_mllama_lm) or elements of `dtype` (mme_load_mllama_lm_as, prepared on the device
 * to the same bits).  The tower lives beside the context's other towers (the tile tower among them); a second load replaces
 * it.  Prepared buffers, in the order mme_weights_fingerprint reports them: embed_tokens bf16 [vocab + 8, hidden], norm f32,
 * projector weight bf16 [hidden, vision_dim], projector bias f32, zeros f32, the rotary cos and sin tables f32 [128, 64]
 * (built on the host), then per layer -- self: input_layernorm f32, q | k | v bf16 [(heads + 2 kv_heads) 128, hidden], o_proj
 * bf16, post_attention_layernorm f32, gate | up bf16 [2 intermediate, hidden], down bf16 -- cross: input_layernorm, q_proj
 * bf16, q_norm f32 [128], k_norm f32 [128], k | v bf16 [2 kv_heads 128, hidden], o_proj * tanh(attn_gate) bf16,
 * post_attention_layernorm, gate | up, down * tanh(mlp_gate) bf16 (tanh on the host, the factor applied in f32 before the
 * rounding to bf16). */
typedef struct mme_mllama_lm_layer {
    int32_t cross;            /* 1: a cross-attention layer (q_norm, k_norm and the gates are read) */
    float attn_gate, mlp_gate; /* cross_attn_attn_gate, cross_attn_mlp_gate: the raw scalars */
    const float *ln1, *ln2;   /* input_layernorm.weight, post_attention_layernorm.weight [hidden] */
    const float *q_w, *k_w, *v_w, *o_w; /* [heads 128, hidden], [kv_heads 128, hidden] x 2, [hidden, heads 128] */
    const float *q_norm, *k_norm;       /* [128] each, cross layers only */
    const float *gate_w, *up_w, *down_w; /* [intermediate, hidden] x 2, [hidden, intermediate] */
} mme_mllama_lm_layer;

typedef struct mme_mllama_lm_weights {
    int32_t hidden, heads, kv_heads, intermediate, layers;
    int32_t vocab;            /* text_config.vocab_size; embed_tokens has vocab + 8 rows */
    int32_t vision_dim;       /* vision_config.vision_output_dim */
    int32_t image_token_id;   /* image_token_index: the id of <|image|> */
    int32_t hidden_act;       /* 0 silu */
    int32_t rope_type;        /* 0 "default", 1 "llama3" */
    int32_t rope_original_max; /* llama3: original_max_position_embeddings */
    float rms_eps, rope_theta, rope_factor, rope_low_freq_factor, rope_high_freq_factor;
    const float *embed_tokens, *norm, *proj_w, *proj_b;
    const mme_mllama_lm_layer* layer; /* [layers] */
} mme_mllama_lm_weights;

int mme_load_mllama_lm(mme_ctx* ctx, const mme_mllama_lm_weights* w);
int mme_load_mllama_lm_as(mme_ctx* ctx, const mme_mllama_lm_weights* w, int dtype, void* stream);
/* out: loaded (0 / 1), hidden, heads, kv_heads, intermediate, layers, cross layers, vocab, vision_dim, image_token_id,
 * rope_type, index in mme_weights_fingerprint's order of the tower's first prepared buffer; all zero before a load */
int mme_mllama_lm_info(mme_ctx* ctx, int32_t out[12]);

/* ids_host int32 [n, S], len_host int32 [n] (attended tokens of each sequence, 1..S: right padding only; under the causal
 * mask nothing behind len - 1 reaches that row, so the padded ids only have to be valid ids).
 * vision_bf16_dev: bf16 [n, tiles, tokens, vision_dim], the vision model's last_hidden_state (padding tiles included), or
 * NULL: the text-only path (tiles, tokens, num_tiles_host and xmask_host are not read).  tiles 1..4, tokens 1..1601.
 * xmask_host uint8 [n, S]: the tiles each row attends, as bits (bit t: tile t; below 1 << tiles).  A row with no bit attends
 * EVERY key (padding tiles included) and its cross layers' MLP term is zero, as transformers computes it.  NULL: the
 * processor's rule -- rows from the first image_token_id on attend tiles [0, num_tiles_host[i]), rows before it none.
 * With vision rows every sequence must hold image_token_id (else MME_E_ARG).
 * emb_f32_dev f32 [n, hidden] and / or emb_bf16_dev bf16 [n, hidden]: the final norm of row len - 1, L2-normalised.
 * Sequences are processed mme_set_chunk (<= 64) at a time; asynchronous on `stream` apart from the staging of the ids. */
int mme_mllama_lm_forward(mme_ctx* ctx, const int32_t* ids_host, const int32_t* len_host, int n, int S, const uint16_t* vision_bf16_dev, int tiles,
                          int tokens, const int32_t* num_tiles_host, const uint8_t* xmask_host, float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);

/* pixel_values -> tile tower -> projector -> language tower, mme_set_chunk (<= 64) images at a time: the first three
 * arguments as mme_tile_vit_forward (both towers loaded, vision_dim == the tile tower's 1280 * (1 + n_intermediate)), the
 * rest as mme_mllama_lm_forward.  The vision states reach the projector as bf16 [chunk, 4, 1601, vision_dim], gathered from
 * the tile tower's own bf16 buffers: the f32 `hidden` tensor of mme_tile_vit_forward is never written.  Bit-identical to
 * mme_tile_vit_forward's hidden (rounded to bf16, which is exact) handed to mme_mllama_lm_forward. */
int mme_mllama_embed(mme_ctx* ctx, const float* pixel_values_dev, const int32_t* aspect_ids_host, const int32_t* num_tiles_host, int n,
                     const int32_t* ids_host, const int32_t* len_host, int S, const uint8_t* xmask_host, float* emb_f32_dev, uint16_t* emb_bf16_dev,
                     void* stream);

/* Diagnostic: ONE launch of a kernel of the language tower (mllama_lm.hip) on the caller's device buffers, synchronous; works
 * on a bare context (tests/test_gpu_mllama_lm.py compares every output element with float64).  bf16 rows; heads are 128 wide.
 *   op 0 gather      x[r] = tok[ids_host[r]], r < rows; tok [vocab, d]
 *      1 rmsnorm     y[r] = bf16(w * (x[r] * rsqrt(mean(x[r]^2) + eps))), rows of d
 *      2 headnorm    in place: the `heads` heads from column col0 on of every row of ld values, each normalised with w [128]
 *      3 rope        in place: rotate_half RoPE on the first `heads` heads of every row of ld values, position r % S;
 *                    cos / sin f32 [128, 64]
 *      4 silu_mul    y [rows, d] = bf16(silu(x[:, :d]) * x[:, d:]), x [rows, 2 d]; rowzero (DEVICE uint8 [rows] or NULL): zero rows
 *      5 pool        row b * S + len_host[b] - 1 of x [n S, d]: w * (x * rstd) in f32, L2 -> emb_f32 / emb_bf16 [n, d]
 *      6 self_attn   x = qkv [n S, (heads + 2 kv_heads) 128] -> y [n S, heads 128], causal, rows at or behind len_host[b] zero
 *      7 cross_attn  x = q [n S, heads 128], kv [n tiles tokens, 2 kv_heads 128], xmask_host uint8 [n S] -> y [n S, heads 128]
 * Preconditions (else MME_E_ARG with a message, nothing launched): pointers non-null and 16-byte aligned; d % 8 == 0 (ops 0, 1,
 * 4), 8..16384; 1 <= S <= 128; heads / kv_heads in {1, 2, 4, 8} (ops 6, 7); ids inside 0..vocab-1; len in 1..S; mask bits
 * below 1 << tiles; ld and col0 cover the heads. */
typedef struct mme_mllama_apply_args {
    const uint16_t* tok;      /* op 0 */
    const int32_t* ids_host;  /* op 0 */
    const int32_t* len_host;  /* ops 5, 6 */
    const uint8_t* xmask_host; /* op 7 */
    uint16_t* x;              /* input (in place for ops 2, 3; output of op 0) */
    uint16_t* y;              /* output of ops 1, 4, 6, 7 */
    const uint16_t* kv;       /* op 7 */
    const float* w;           /* ops 1, 2, 5 */
    const float *cos, *sin;   /* op 3 */
    const uint8_t* rowzero;   /* op 4 */
    float* emb_f32;           /* op 5 */
    uint16_t* emb_bf16;
    int64_t rows, ld;
    int32_t n, S, d, heads, kv_heads, col0, vocab, tiles, tokens;
    float eps;
} mme_mllama_apply_args;
int mme_mllama_apply(mme_ctx* ctx, int op, const mme_mllama_apply_args* args, void* stream);

/* ---- multi-GPU: the ONE exchange step of the path ------------------------------------------
 * Replaces the hand-back of per-device results through Python lists by the reference's thread pool
 * (deprecated_package/embedder.py:208-224): every rank embeds its contiguous block of the corpus and the
 * [rows, d] bf16 shards are all-gathered over RCCL (xGMI) so that each rank can compute its row block of the
 * cosine matrix / its page pairs / its neighbour lists against all N rows.
 *   mme_comm_unique_id  rank 0 makes the 128-byte rendezvous id and hands it to the other ranks by any
 *                       means (a file, MPI, a socket);
 *   mme_comm_init       every rank, collectively: communicator for this context's GPU;
 *   mme_allgather       all[r * rows .. (r+1) * rows) = rank r's shard, asynchronous on `stream`;
 *                       equal shards (pad the last rank's block: rows are independent);
 *   mme_comm_destroy.
 * `comm` is an ncclComm_t: a communicator the caller created itself with RCCL works as well.  RCCL is resolved
 * at run time (the copy PyTorch loaded, else librccl.so.1; MME_RCCL_LIB overrides) -- libmme.so does not link it,
 * and a missing RCCL only fails these four calls (MME_E_COMM). */
#define MME_COMM_ID_BYTES 128
int mme_comm_unique_id(mme_ctx* ctx, uint8_t id_host[MME_COMM_ID_BYTES]);
int mme_comm_init(mme_ctx* ctx, const uint8_t id_host[MME_COMM_ID_BYTES], int rank, int world, void** comm_out);
int mme_comm_destroy(mme_ctx* ctx, void* comm);
int mme_allgather(mme_ctx* ctx, void* comm, const uint16_t* shard_dev, int64_t rows, int d, uint16_t* all_dev, void* stream);

/* ---- timing of the kernels by class (HIP events on the launch stream) ----------------------
 * class ids: 0 preprocess, 1 gemm, 2 layernorm, 3 attention, 4 pool, 5 cosine, 6 page_reduce, 7 cluster,
 * 8 neighbours, 9 all-gather */
#define MME_NUM_KERNEL_CLASSES 10
int mme_profile_enable(mme_ctx* ctx, int on);
int mme_profile_reset(mme_ctx* ctx);
/* synchronises the recorded events; ms[c] = total ms, launches[c] = launch count per class, for the first
 * min(count, MME_NUM_KERNEL_CLASSES) classes: `count` is the capacity of BOTH caller arrays, so a binder built against
 * a header with fewer classes is never overrun.  Returns the number of classes the library knows (>= 0) or MME_E_*. */
int mme_profile_read_sync(mme_ctx* ctx, int count, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* MME_H */
