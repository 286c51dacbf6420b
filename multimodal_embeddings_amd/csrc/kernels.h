// Launcher declarations shared between the kernel translation units and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_bits;  // host-visible alias; device code uses __bf16

enum GemmEpilogue {
    EPI_BIAS = 0,       // out = bf16(acc + bias[n])                                  (QKV)
    EPI_BIAS_GELU = 1,  // out = bf16(gelu_erf(acc + bias[n]))                        (fc1)
    EPI_BIAS_RES = 2,   // out = bf16(acc + bias[n] + res[m,n])   (res may alias out) (o_proj, fc2)
    EPI_PATCH = 3,      // row m=(b,p) -> out row b*197+1+p, + bias[n] + pos[1+p,n]   (patch embed)
    EPI_F32 = 4,        // outf[m,n] = acc                                            (cosine)
    // LayerNorm folded into the GEMM that consumes it (A = the raw residual stream x, W' = W*gamma):
    //   out = bf16(rstd[m] * (acc - mean[m] * colsum[n]) + bias'[n])             (QKV)
    EPI_LN_BIAS = 5,
    EPI_LN_BIAS_GELU = 6, // same, then erf-GELU                                      (fc1)
    EPI_TOPK = 7,         // no output matrix: every acc[m,n] >= thr[m] is appended to row m's candidate list (K12)
    // EPI_BIAS_RES that also leaves, per output row and 64-column slice, the LayerNorm partial sums (sum x, sum x^2 of
    // the ROUNDED outputs) in ln_part: the next LayerNorm's statistics then need no pass over the residual stream
    EPI_BIAS_RES_STATS = 8,
    // QuickGELU, x * sigmoid(1.702 x), where the erf forms have erf-GELU (CLIP image towers with OpenAI weights)
    EPI_BIAS_QGELU = 9,     // out = bf16(quick_gelu(acc + bias[n]))                      (fc1, LayerNorm-kernel mode)
    EPI_LN_BIAS_QGELU = 10, // EPI_LN_BIAS, then QuickGELU                                (fc1)
    // tanh-GELU, 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) (gelu_pytorch_tanh: SigLIP image towers)
    EPI_BIAS_TGELU = 11,    // out = bf16(gelu_tanh(acc + bias[n]))                       (fc1, LayerNorm-kernel mode)
    EPI_LN_BIAS_TGELU = 12  // EPI_LN_BIAS, then tanh-GELU                                (fc1)
};

struct GemmArgs {
    const void* A;   // bf16 [M, K] row-major
    const void* W;   // bf16 [N, K] row-major ("TN": both operands K-contiguous)
    int M, N, K;     // valid extents; K % 64 == 0
    const float* bias;
    void* out;       // bf16
    int64_t ldo;
    const void* res; // bf16, same layout as out
    const float* pos;
    float* outf;
    int64_t ldf;
    const float* ln_stats;  // [M,2] (mean, rstd) per row, for EPI_LN_*
    float* ln_part;         // EPI_BIAS_RES_STATS: [2][N/64][ln_part_rows] f32 partial (sum, sum of squares) planes
    int64_t ln_part_rows;
    const float* colsum;    // [N] sum_k W'[n,k], for EPI_LN_*
    // EPI_TOPK: per-row threshold thr[m * thr_stride]; candidates (value, column) of row m go to
    // cand_val / cand_idx [m * cand_cap + k], k = atomic slot from cand_count[m]; a full list raises *overflow
    const float* thr;
    int thr_stride;
    int* cand_count;
    float* cand_val;
    int* cand_idx;
    int cand_cap;
    int* overflow;
    const int* run_if;      // optional: the whole launch is a no-op unless *run_if != 0 (device-side fallback switch)
    int reverse_m;          // 256 x 256 kernel: walk the row panels from the LAST one down (same results; zig-zag: EncoderPass::zigzag, encoder_pass.h)
};

// raises hipFuncAttributeMaxDynamicSharedMemorySize of `kernel` on the CURRENT device to at least `bytes`
// (once per (device, kernel), thread-safe: launch_state.hip)
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);

hipError_t launch_gemm(int epilogue, const GemmArgs& g, hipStream_t s, int variant = 0);
// diagnostic: stamped build of the 3-deep-ring 256x256 kernel (bias epilogue), stamps uint64[256 * 2 * 16]
hipError_t launch_gemm256r_stamped(const GemmArgs& g, unsigned long long* stamps, hipStream_t s);

// LayerNorm over bf16 rows of d (f32 statistics), bf16 out.  d: a width the row kernels are instantiated for (384, 768,
// 1024; common.h vit_width_built), as for launch_ln_stats, launch_cls_rows and launch_pool; else hipErrorInvalidValue
hipError_t launch_layernorm(const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int d, float eps, hipStream_t s);
// the same LayerNorm IN PLACE on rows [0, rows) of x, and stats[row] = (mean, rstd) of the ROUNDED result in the canonical
// summation order: bit-identical to launch_ln_stats_canonical on x afterwards (CLIP's pre_layrnorm, the statistics source
// of the pass's first folded LayerNorm)
hipError_t launch_pre_ln(void* x, const float* gamma, const float* beta, int64_t rows, int d, float eps, float* stats, hipStream_t s);
// The launchers that take `tokens` look the layout up in the table of layouts.h and refuse (hipErrorInvalidValue) a count
// that is no row, or a row without the operation.
// LayerNorm of row b*tokens+tok of d values -> bf16 [B, d] (launch_pool without its L2 step: CLIP's post_layernorm);
// tokens: an image layout with a pooled row (197, 50, 257), 0 <= tok < tokens
hipError_t launch_pool_ln(const void* x, const float* gamma, const float* beta, int B, int tokens, int tok, int d, float eps, void* y, hipStream_t s);
// x / max(||x||, 1e-12) as f32 and/or bf16 [rows, p]; p % 64 == 0, p <= 1024.  x: f32 [rows, p]; bf16 [rows, p], widened;
// or acc f32 [rows, p] + bias [p] (the rows of a GEMM under EPI_F32), the sum formed once in f32
hipError_t launch_l2_rows(const float* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s);
hipError_t launch_l2_rows_bf16(const void* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s);
hipError_t launch_bias_l2_rows(const float* acc, const float* bias, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s);
// per-row LayerNorm statistics of bf16 rows of d: stats[row] = (mean, rstd)
hipError_t launch_ln_stats(const void* x, int64_t rows, int d, float eps, float* stats, hipStream_t s);
// the same statistics in the CANONICAL summation order shared with the EPI_BIAS_RES_STATS epilogue, for rows
// [row0, row1) of bf16 rows of `d` (d % 64 == 0, d <= 2048): one pass over x
// rows row0, row0 + stride, ... < row1
hipError_t launch_ln_stats_canonical(const void* x, int64_t row0, int64_t row1, int d, float eps, float* stats, hipStream_t s, int64_t stride = 1);
// finishes rows [0, rows) from the partial planes an EPI_BIAS_RES_STATS GEMM left: part [2][d/64][part_rows]
hipError_t launch_ln_finish(const float* part, int64_t part_rows, int64_t rows, int d, float eps, float* stats, hipStream_t s);
// true when launch_gemm(variant) runs a large-tile kernel (256 x 256 or 384 x 256), whose fast-path epilogue writes the partial planes
bool gemm_runs_256(const GemmArgs& g, int variant);
// rows [0, this) lie in the interior row tiles of the kernel launch_gemm(epilogue, g, s, variant) runs (256- or 384-row
// tiles; 0 for the 128 x 128 kernel): the rows whose partial planes an EPI_BIAS_RES_STATS / EPI_PATCH launch leaves
int64_t gemm_interior_rows(int epilogue, const GemmArgs& g, int variant);
// x[b*197 + 0, :] = bf16(cls + pos[0]), rows of d
hipError_t launch_cls_rows(void* x, const float* cls, const float* pos, int B, int d, hipStream_t s);
// final LayerNorm on row b*tokens+tok of d values, L2 normalise, write f32 and/or bf16 [B, d]; tokens and tok as launch_pool_ln
hipError_t launch_pool(const void* x, const float* gamma, const float* beta, int B, int tokens, int tok, int d, float eps,
                       float* emb_f32, void* emb_bf16, hipStream_t s);
// launch_pool over a window of rows per crop: final LayerNorm + L2 of rows b*tokens + tok0 .. + ntok - 1 -> y bf16 [n, ntok, d], each
// row K8's bf16 output for that pool token bit for bit; tokens: any image layout, 0 <= tok0, 1 <= ntok, tok0 + ntok <= tokens
hipError_t launch_token_rows(const void* x, const float* gamma, const float* beta, int n, int tokens, int tok0, int ntok, int d, float eps, void* y,
                             hipStream_t s);
// Mean pooling over the covered patch tokens (pooling.hip): the final LayerNorm of the rows first + r * g + c,
// r < R, c < C, of crop b, their f32 mean m in the fixed order of pooling.hip, then m / max(||m||, 1e-12) -> [B, d], or under
// cls_mean [y_0 | m] / max(||.||, 1e-12) -> [B, 2 d] (f32 and / or bf16).  grids: DEVICE int32 [B, 2] (R, C), each 1..g (the
// caller validates; the kernel clamps), or null: (g, g) for every crop.  tokens == first + g * g, g <= 16, first 0 or 1 (1 under
// cls_mean), d as launch_pool; else hipErrorInvalidValue
hipError_t launch_pool_mean(const void* x, const float* gamma, const float* beta, const int32_t* grids, int B, int tokens, int g, int first,
                            bool cls_mean, int d, float eps, float* emb_f32, void* emb_bf16, hipStream_t s);
// behind a patch-embed GEMM under EPI_F32 (acc f32 [n * patches, d]), one rounding per value: with a class token (cls
// non-null; tokens = 50 or 257) x[b*tokens + 1 + p] = bf16((acc + bias) + pos[1 + p]) and x[b*tokens] = bf16(cls + pos[0]);
// without one (cls null; tokens = patches = 196) x[b*tokens + p] = bf16((acc + bias) + pos[p]).  tokens: an image layout whose
// row sets embed_rows, cls non-null exactly when it has a class row
hipError_t launch_embed_rows(const float* acc, const float* bias, const float* pos, const float* cls, void* x, int n, int tokens, int d, hipStream_t s);
// f32 [rows,d] -> L2-normalised bf16 [rows,d]
hipError_t launch_normalise_rows(const float* x, int64_t rows, int d, void* y, hipStream_t s);
// fused multi-head attention of the layouts of attention.hip (197 tokens, or 196: towers without a class token), dh=64, `heads` = 6, 12
// or 16 (one instantiation each); qkv [B*tokens, 3*64*heads] -> out [B*tokens, 64*heads].  Anything else is hipErrorInvalidValue
// guard: device int, zero before the launch; non-null selects the FAST kernel + the conditional exact re-run (attention.hip)
// force_redo: the fast kernel raises the guard for every row (test of the re-run path)
// only_block >= 0: compute and store that query block of 32 only (0..6)
// reverse: walk the crops from the last one down (same results; zig-zag order of consecutive kernels, EncoderPass::zigzag)
hipError_t launch_attention(const void* qkv, void* out, int B, int heads, hipStream_t s, int* guard = nullptr, bool force_redo = false,
                            int only_block = -1, bool reverse = false, int tokens = 197);
// diagnostic: stamped build of the fast or the exact form, stamps uint64[B][8][8]
hipError_t launch_attention_stamped(const void* qkv, void* out, int B, int heads, bool fast, unsigned long long* stamps, hipStream_t s);

struct CropDesc {  // one per crop, built on the host (k1_plan.h: plan_crop)
    int64_t src_off;   // byte offset into pix
    int64_t tmp_off;   // byte offset (16-aligned) into the horizontal-pass scratch (if the width changes)
    int64_t tab_off;   // byte offset (16-aligned) of this crop's resampling tables in the table buffer (K1Layout)
    int32_t h, w;      // source size
    int32_t new_h, new_w;
};
struct HWork {  // one block of the horizontal pass: a band of source rows of one crop
    int32_t crop, row0, nrows;
};
// Row pitch of the horizontal pass's scratch image: rows start 16-byte aligned so the vertical pass reads them as dwords
// (four adjacent output bytes per LDS read) and stages them with 16-byte copies.
__host__ __device__ inline int k1_tmp_pitch(int new_w) { return (new_w * 3 + 15) & ~15; }
// Resampling tables of one crop (resample_tables), at tab + crop.tab_off:
//   width changes:  Taps[new_w] {xmin, n} | pad to 16 | uint4 hk[gh][new_w]   -- coefficients in groups of four taps,
//                   group-major so that adjacent output columns read adjacent 16-byte words; zero beyond tap n
//   height changes: Taps[new_h] | pad to 16 | int vk[new_h][kv]               -- zero beyond tap n
// gh * 4, kv >= 2 * ceil(scale) + 1 = Resample.c's ksize, the upper bound of n.  The integer formulas below (k1_h_groups, kv
// of k1_layout) equal resample_ksize<Triangle> (resample.h) rounded up to a multiple of four: ceil(max(w / new_w, 1)) is the
// integer ceiling of w / new_w (1 for an enlarged axis in both); they stay integer so that a layout function does not
// depend on f64.
// Held over every admitted size (1..8000 x 1..8000) by tests/test_k1_plan_cpu.py, which also finds the attained maxima: under
// fit-and-pad ksize <= 143, gh <= 36, kv <= 144 (a 70 x 7841 crop becomes one row), and a window's true length never exceeds ksize.
// groups of four taps per output column of the horizontal pass
__host__ __device__ inline int k1_h_groups(int w, int new_w) { return (2 * ((w + new_w - 1) / new_w) + 1 + 3) >> 2; }
// bytes of LDS the horizontal table of a crop takes beside its band (table padded to whole 1 KiB DMA sweeps)
__host__ __device__ inline int k1_h_table_lds(int w, int new_w) {
    return ((((new_w * 8 + 15) & ~15) + k1_h_groups(w, new_w) * new_w * 16) + 1023) & ~1023;
}
struct K1Layout {
    int gh, kv;
    int64_t hk_off, vt_off, vk_off, bytes;
};
__host__ __device__ inline K1Layout k1_layout(int h, int w, int new_h, int new_w) {
    K1Layout L;
    const bool hp = new_w != w, vp = new_h != h;
    L.gh = hp ? k1_h_groups(w, new_w) : 0;
    L.kv = vp ? ((2 * ((h + new_h - 1) / new_h) + 1 + 3) & ~3) : 0;
    L.hk_off = hp ? (((int64_t)new_w * 8 + 15) & ~(int64_t)15) : 0;
    L.vt_off = L.hk_off + (int64_t)L.gh * new_w * 16;
    L.vk_off = L.vt_off + (vp ? (((int64_t)new_h * 8 + 15) & ~(int64_t)15) : 0);
    L.bytes = (L.vk_off + (int64_t)new_h * L.kv * 4 + 15) & ~(int64_t)15;
    return L;
}
constexpr int K1_H_RPT = 8;       // source rows one item of the horizontal pass filters (bands are whole groups of them)
constexpr int K1_H_RPT_WIDE = 4;  // ... in the second launch (crops whose table + eight rows do not fit the LDS budget)
// both tap tables of every crop, once per crop (f64 on the device exactly as Resample.c computes them on the host)
hipError_t launch_resample_tables(const CropDesc* crops, int n, uint8_t* tab, hipStream_t s);
// horizontal pass over `nwork` bands of ONE class (k1_plan.h: K1Plan): 0 = eight-row items, table in LDS beside the band;
// 1 = four-row items, table in LDS; 2 = four-row items, table through L1.  lds_bytes = the largest (table +) band.
// (launch_resize_h and launch_clip_resize_h are the one kernel template of resample.h over the two descriptors.)
hipError_t launch_resize_h(const uint8_t* pix, uint8_t* tmp, const CropDesc* crops, const HWork* work, int nwork, int lds_bytes,
                           int cls, const uint8_t* tab, hipStream_t s);
// multi-tile Mllama output: grid_of int32[n,2] (tiles_h, tiles_w); out f32 [n, max_tiles, 3, T, T]
hipError_t launch_resize_v_tiles(const uint8_t* pix, const uint8_t* tmp, const CropDesc* crops, const int32_t* grid_of, int n,
                                 const float* lut, float* out, int T, int max_tiles, hipStream_t s);
// K0: boxes int32[n,4] (x0,y0,x1,y1), offs int64[n] byte offsets into pix; zero fill outside the page
hipError_t launch_crop_boxes(const uint8_t* page, int H, int W, const int32_t* boxes, const int64_t* offs, const HWork* work, int nwork,
                             uint8_t* pix, hipStream_t s);
// bf16(lut[c][u]) == bf16(fma(u, a[c], b[c])) for all 256 u and the 3 channels, VERIFIED on the host when the table was
// built (capi.hip, set_lut): the patch emitter then computes the value instead of reading the table at 64 data-dependent
// LDS addresses per instruction (47 % of that kernel's LDS cycles were bank conflicts, profiles/round2_pmc_k1_sq.csv).
// exact == 0: no such pair was found for this mean / std -- the emitter keeps the table.
struct NormAffine {
    float a[3], b[3];
    int exact;
};
hipError_t launch_resize_v_patchify(const uint8_t* pix, const uint8_t* tmp, const CropDesc* crops, int n,
                                    const float* lut /*[3,256]*/, const NormAffine& aff, void* patches, bool any_resize, const uint8_t* tab, int kv_max,
                                    hipStream_t s);

// ---- K1 under MME_RESIZE_CLIP and MME_RESIZE_SPEC (preprocess_clip.hip, on resample.h): a resize of the whole crop (CLIP's:
// shortest edge 224, BICUBIC; a spec's: mme_resize_spec) + centre crop, only the 224 x 224 window of the resized image
// computed.  What CropDesc cannot carry: the FULL resized sizes, the window's origin and the
// source rows the horizontal pass filters.
struct ClipCropDesc {  // one per crop, built on the host (k1_plan.h: plan_spec_crop)
    int64_t src_off;       // byte offset into pix
    int64_t tmp_off;       // byte offset (16-aligned) of this crop's scratch image: nr rows of 672 bytes
    int64_t tab_off;       // byte offset (16-aligned) of this crop's tables (ClipLayout)
    int32_t h, w;          // source size
    int32_t new_h, new_w;  // size of the whole resized image (CLIP: 224 on the short edge, int(224 * long / short) on the other)
    int32_t top, left;     // origin of the centre-crop window in the resized image
    int32_t r0, nr;        // source rows [r0, r0 + nr): the union of the 224 vertical windows (rows top.. when the height is kept)
    int32_t gh, kv;        // groups of four taps per output column; ints per vertical coefficient row (a multiple of 4)
};
// Tables of one crop (clip_tables), at tab + crop.tab_off; both axes hold exactly 224 output coordinates:
//   Taps[224] {xmin, n} source columns | int4 hk[gh][224], group-major, zero beyond tap n
//   Taps[224] {xmin, n} scratch rows (source row - r0) | int vk[224][kv], zero beyond tap n
// An axis whose size does not change holds one-tap windows of weight 2^22 (an exact copy).
struct ClipLayout {
    int64_t hk_off, vt_off, vk_off, bytes;
};
__host__ __device__ inline ClipLayout clip_layout(int gh, int kv) {
    ClipLayout L;
    L.hk_off = 224 * 8;
    L.vt_off = L.hk_off + (int64_t)gh * 224 * 16;
    L.vk_off = L.vt_off + 224 * 8;
    L.bytes = L.vk_off + (int64_t)224 * kv * 4;
    return L;
}
// bytes of LDS the horizontal table takes beside a band (padded to whole 1 KiB DMA sweeps)
__host__ __device__ inline int clip_h_table_lds(int gh) { return (224 * 8 + gh * 224 * 16 + 1023) & ~1023; }
// `resample`: Pillow's number of the filter, 2 (BILINEAR: Triangle) or 3 (BICUBIC)
hipError_t launch_clip_tables(const ClipCropDesc* crops, int n, uint8_t* tab, int resample, hipStream_t s);
// horizontal pass over `nwork` bands of one class, as launch_resize_h: 0 = eight-row items, table in LDS; 1 = four-row
// items, table in LDS; 2 = four-row items, table through L1.  HWork::row0 is a SOURCE row (>= r0).
hipError_t launch_clip_resize_h(const uint8_t* pix, uint8_t* tmp, const ClipCropDesc* crops, const HWork* work, int nwork, int lds_bytes,
                                int cls, const uint8_t* tab, hipStream_t s);
hipError_t launch_clip_v_patchify(const uint8_t* tmp, const ClipCropDesc* crops, int n, const float* lut /*[3,256]*/, const NormAffine& aff,
                                  void* patches, const uint8_t* tab, int kv_max, hipStream_t s);

// K13: class-aware greedy NMS, one workgroup per page (3_combine_grids.py:80-137).  boxes f64[n,4] (x0,y0,x1,y1),
// page p owns boxes [page_offs[p], page_offs[p+1]); order int32[n] is scratch; keep int32[n] receives, per page, the
// page-local indices of the kept boxes in the reference's output order (-1 beyond keep_count[p]).  <= 32768 boxes per page.
hipError_t launch_nms_pages(const double* boxes, const double* scores, const int32_t* classes, const int32_t* page_offs, int pages,
                            double thr, int32_t* order, int32_t* keep, int32_t* keep_count, hipStream_t s);

struct PageSimArgs {
    const void* emb;        // bf16 [N, d]
    int64_t N;
    int d;
    const double* area_pct; // [N]
    const uint8_t* valid;   // [N]
    const int32_t* page_offs; // device [P+1]
    int P;
    const uint8_t* skip;    // [P,P] or null
    int max_query, top_k;
    double max_dist;
    int metric, normalise;
    int64_t pair_lo, pair_hi; // upper-triangle pair ranks [lo, hi) computed by this call (multi-GPU shards); hi < 0 = all
    double* S;              // [P,P]
    // workspace
    float* qsim;            // [nq, N] f32
    const int32_t* qrow;    // device [nq] row index of each query region
    const int32_t* qpage;   // device [nq]
    const int32_t* qstart;  // device [P+1] first query of each page
    int nq;
    void* qemb;             // bf16 [nq, d] gathered query rows
    double* maxbuf;         // [1]
};
hipError_t launch_page_similarity(const PageSimArgs& a, hipStream_t s);

// K12 ranked neighbour lists (neighbours.hip): one wave per row of qsim[nrows, ld] keeps the best `fetch`
// entries in (similarity desc, index asc) order, then filters self / group / score window into top_n
hipError_t launch_topk_rows(const float* qsim, int64_t ld, int N, int nrows, int row0, const int32_t* group, int fetch, int top_n,
                            int keep_self, float min_sim, float max_sim, int32_t* idx_out, float* sim_out, hipStream_t s,
                            const int* run_if = nullptr);
// the same selection over per-row candidate lists (value, column id) produced by the EPI_TOPK GEMM epilogue
hipError_t launch_topk_candidates(const float* cand_val, const int32_t* cand_idx, const int32_t* len, int cap, int nrows, int row0,
                                  const int32_t* group, int fetch, int top_n, int keep_self, float min_sim, float max_sim,
                                  int32_t* idx_out, float* sim_out, hipStream_t s);

// K11 page clustering (cluster.hip): labels_out int32[P], k_out int32[1], scores_out double[16]
hipError_t launch_cluster(const double* S, int P, int n_clusters, int mode, char* ws, int32_t* labels_out, int32_t* k_out,
                          double* scores_out, hipStream_t s);
size_t cluster_workspace_bytes(int P);

// RCCL, resolved at run time (comm.hip)
const char* rccl_ready();  // nullptr = usable, else why not
const char* rccl_error_string(int code);
int rccl_unique_id(void* id128);
int rccl_comm_init(void** comm, int world, const void* id128, int rank);
int rccl_comm_destroy(void* comm);
int rccl_allgather_bytes(const void* send, void* recv, size_t bytes, void* comm, hipStream_t s);

// ---- tile-ViT encoder (tilevit.hip, attention_tiles.hip): Mllama vision tower geometry, fixed at compile time:
// 4 tiles x (1601 -> 1608) tokens, 1280-d, 16 heads of 80, patch 14 on 560 x 560 tiles
hipError_t launch_tile_patchify(const float* pv, void* patches, int64_t npatch, hipStream_t s);
hipError_t launch_tile_assemble(const void* pemb, const float* cls, const float* pre, const float* pos, const float* tilepos, const float* g,
                                const float* b, const int32_t* aid, void* x, int64_t rows, float eps, hipStream_t s);
hipError_t launch_tile_ln_post(void* x, const float* g, const float* b, const float* post, const int32_t* aid, int64_t rows, float eps, hipStream_t s);
hipError_t launch_tile_output(const void* x, const void* inter, int ni, int64_t inter_stride, float* hidden, int64_t out_rows, hipStream_t s);
hipError_t launch_tile_pool(const void* x, const void* inter, int ni, int64_t inter_stride, int n, float* emb_f32, void* emb_bf16, hipStream_t s);
hipError_t launch_attention_tiles(const void* qkv, void* out, const int32_t* ntiles_dev, int n, hipStream_t s, int* guard = nullptr, bool force_redo = false);

// ---- the text towers (text_tower.hip, attention_short.hip): 77 tokens under a causal mask (CLIP) or 64 without a mask (SigLIP:
// last-token pooling and a head with bias, launch_bias_l2_rows); heads of 64, d = 512, 768 or 1024 (else hipErrorInvalidValue).
// tokens: a text layout of the table
// x[b*T + t, :] = bf16(f32(tok[ids[b*T + t], :]) + pos[t, :]); tok bf16 [vocab, d], pos f32 [T, d], ids DEVICE int32 [n*T], each
// 0 <= id < vocab (the caller validates them on the host)
hipError_t launch_text_token_rows(const void* tok, const float* pos, const int32_t* ids, void* x, int n, int d, hipStream_t s, int tokens = 77);
// LayerNorm (launch_pool_ln's) of row b*tokens + eos_pos[b] (DEVICE int32 [n], each 0..tokens-1) -> y bf16 [n, d] and / or y_f32 [n, d];
// the SigLIP tower pools position 63 of every sequence
hipError_t launch_text_eos_pool_ln(const void* x, const float* gamma, const float* beta, const int32_t* eos_pos, int n, int d, float eps, void* y,
                                   float* y_f32, hipStream_t s, int tokens = 77);
// out[i] = 1 / (1 + exp(-(cos[i] * scale + bias))), i < count; out may be cos
hipError_t launch_siglip_scores(const float* cos, float* out, int64_t count, float scale, float bias, hipStream_t s);

// ---- exact attention of the layouts outside attention.hip (attn_short<T, CAUSAL>: 77 causal, 50, 64; attn_mid: 257): dh = 64,
// qkv [n*T, 3*64*heads] (Q pre-scaled by dh^-0.5 log2 e) -> out [n*T, 64*heads], exact row maximum.  heads: the layout's set;
// only_block = -1, or a query block of 32 below the layout's `blocks` (that block only; the causal layout takes -1 only)
hipError_t launch_attention_exact(const void* qkv, void* out, int n, int tokens, bool causal, int heads, hipStream_t s, int only_block = -1);
hipError_t launch_attn_mid(const void* qkv, void* out, int n, int heads, hipStream_t s, int only_block);  // attention_mid.hip, behind it: checked arguments, n > 0

// ---- K1's bf16 patch-16 matrix [n * 196, 768] -> the patch matrix of another patch size in conv order (c, ky, kx):
// patch 32 (patch32.hip): [n * 49, 3072], a pure copy; patch 14 (dinov2.hip): [n * 256, 640], a 2-byte gather, columns 588..639
// zero on every launch.  Any other patch is hipErrorInvalidValue
hipError_t launch_retile(int patch, const void* patches16, void* dst, int n, hipStream_t s);

// ---- SigLIP ViT/16 @224 image towers (siglip.hip; attention: launch_attention with tokens = 196; launch_embed_rows without a
// class row; launch_l2_rows_bf16 behind the head): 196 tokens, no class token
// attention pooling: kv bf16 [n*196, 2*64*heads] (K | V), q f32 [64*heads] (pre-scaled by dh^-0.5 log2 e, the same for every
// crop) -> out bf16 [n, 64*heads]; exact maximum, f32 sums, one rounding; heads = 6, 12 or 16
hipError_t launch_map_pool(const void* kv, const float* q, void* out, int n, int heads, hipStream_t s);

// ---- device-side weight preparation (weight_prep.hip).  dt = MME_DT_* (include/mme.h); sources are device addresses,
// 16-byte aligned, of elements of that type.
// `count` elements (a multiple of 8) -> f32 table or bf16 (round to nearest even) at dst (16-byte aligned);
// `scaled`: every value times `scale` (in f32) first
hipError_t launch_wp_convert(int dt, const void* src, size_t count, float scale, bool scaled, bool out_bf16, void* dst, hipStream_t s);
// [rows, cols] -> bf16 [rows, cols_padded] with zero columns behind (cols, cols_padded multiples of 4)
hipError_t launch_wp_pad(int dt, const void* src, int rows, int cols, int cols_padded, void* dst_bf16, hipStream_t s);
struct WpFoldSrc {
    const void* w;  // [rows, cols]
    const void* b;  // [rows] or null: no bias
    float scale;
    int scaled;     // weights and bias times `scale`, rounded to f32, before anything else (the query rows)
};
// LayerNorm folding of up to three row blocks (rows[i] multiples of 64; cols a multiple of 64, <= 1280):
// wf bf16 [sum rows, cols], cs / bf f32 [sum rows]; sums over k ascending in f64, a row per thread
// [rows, cols] (cols a multiple of 8) times a per-row factor: dst bf16 [rows, cols] = bf16_rne(f32(factor[row] * src[row, col]))
hipError_t launch_wp_rowscale(int dt, const void* src, size_t rows, size_t cols, const void* factor, void* dst_bf16, hipStream_t s);
// f32 table dst[i] = f32(factor[i] * src[i]), any n
hipError_t launch_wp_mul(int dt, const void* src, const void* factor, size_t n, float* dst, hipStream_t s);
hipError_t launch_wp_fold(int dt, const WpFoldSrc* srcs, const size_t* rows, int nsrc, int cols, const void* gamma, const void* beta, void* wf, float* cs,
                          float* bf, hipStream_t s);
