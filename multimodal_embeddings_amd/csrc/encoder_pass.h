// One pre-LN transformer block as every encoder of the library runs it (encoder_pass.hip): the image towers
// (image_tower.hip), the text towers (capi_text.hip) and the tile-ViT (capi_tilevit.hip) differ in the settings of
// EncoderPass and in the attention launch they put between the block's two halves, not in the sequence.
#pragma once
#include "ctx.h"

// What one pass of one tower is run with.  The towers fill it once per chunk; `dir` is the only field the block changes.
struct EncoderPass {
    mme_ctx* c;
    hipStream_t s;
    int D, F;       // hidden width, MLP width
    float eps;
    int act;        // fc1's activation: 0 erf-GELU, 1 QuickGELU, 2 tanh-GELU
    // workspace: residual stream, Q | K | V, attention output, MLP hidden (bf16); (mean, rstd) per row
    void *x, *qkv, *att, *mlp;
    float* stats;
    // Non-null selects the LayerNorm-kernel form of the two halves (ln_mode 0, image towers only): the buffer [rows, D]
    // the normalised rows are written to.  Null: every LayerNorm is folded into the GEMM that consumes it.
    void* hbuf = nullptr;
    bool unfolded() const { return hbuf != nullptr; }
    // Partial (sum, sum of squares) planes [2][D/64][lnpart_rows] that the residual GEMMs are handed (null: none).
    // `planes` says whether they are USED: the GEMMs that write x then run EPI_BIAS_RES_STATS and the statistics of the
    // rows their interior tiles wrote are finished from the planes (96 bytes per row at D = 768) instead of read from x.
    float* lnpart;
    int64_t lnpart_rows;
    bool planes;
    // Zig-zag: consecutive kernels of the pass walk the rows in OPPOSITE directions, so a consumer starts on the rows its
    // producer wrote last -- what is still in the 256 MiB Infinity Cache of a 1.2-5 GB activation -- instead of on the rows
    // written first and long evicted.  Tile order only: results are bit-identical (tests).
    int zigzag;   // 0 off, 1 every kernel alternates (dir flips at every producer), 2 only the attention walks backwards
    int dir = 0;  // the direction the last kernel walked
    int next_dir() {
        if (zigzag == 1) dir ^= 1;
        return dir;
    }
    // The same pass on a handful of gathered rows (a pruned last layer, SigLIP's head): far below one 256-row panel,
    // so no planes and one canonical statistics pass, and no reversal
    EncoderPass on_few_rows() const {
        EncoderPass g = *this;
        g.lnpart = nullptr;
        g.planes = false;
        g.zigzag = g.dir = 0;
        return g;
    }

    // one launch in one KC_GEMM scope
    int gemm(int epilogue, const GemmArgs& g);
    // statistics of rows [row0, rows) of `xr` in the canonical summation order: one read of those rows
    int stats_from_x(const void* xr, int64_t row0, int64_t rows);
    // statistics of the `rows` rows `producer` wrote (producer.out): the rows of the interior row tiles of the kernel that
    // ran (gemm_interior_rows: 256- or 384-row tiles) are finished from the planes when they are used and the launch ran a
    // large-tile kernel (the only ones that leave them), the ragged tail -- or, otherwise, every row -- takes
    // stats_from_x, which sums in the same order: the same bits either way
    int stats_after(const GemmArgs& producer, int64_t rows);
    // out = xr + a . w^T + bias on `rows` rows (o_proj, fc2), in place on xr; `stats_next`: a folded LayerNorm reads xr next
    int residual(const void* a, const bf16_t* w, const float* bias, int K, int rows, void* xr, bool stats_next);
    // first half, folded: qkv [rows, N] = LN1(x) . qkv_w^T + b (statistics of x are in `stats`); N = 3 D, or 2 D for the
    // K | V projection of SigLIP's head
    int qkv_ln(const BlockW& w, int rows, int N);
    // fc1 with LN2 folded in and the activation: mlp = act(LN2(xr) . fc1_w^T + b)
    int fc1_ln(const BlockW& w, int rows, const void* xr);
    // second half, after the tower's attention launch: o_proj + residual, statistics, fc1, fc2 + residual, and the
    // statistics again when `stats_next` (the next block's QKV GEMM reads them).  `a` [rows, D] is the attention output
    // and `xr` [rows, D] the residual rows: the pass's own buffers, or the gathered rows of a pruned last layer
    int after_attention(const BlockW& w, int rows, const void* a, void* xr, bool stats_next);
    // The two halves of an image-tower layer in the form the pass runs.  Folded: qkv_ln / after_attention on L.w.
    // Unfolded: a LayerNorm launch (gamma, beta -> hbuf) in front of EPI_BIAS into qkv; o_proj + residual, a LayerNorm
    // launch (ln2), fc1 with its activation, fc2 + residual -- no statistics, `stats_next` is not consulted.
    int layernorm(const void* xr, const float* gamma, const float* beta, int rows);  // xr -> hbuf, one KC_LN scope
    int first_half(const LayerDev& L, const float* gamma, const float* beta, int rows, int N);
    int second_half(const LayerDev& L, int rows, const void* a, void* xr, bool stats_next);
};

// one guard word per layer for the fast attention forms (attention.hip, attention_tiles.hip), zeroed per pass -- in
// attention mode 0 too, so that mme_attention_redone reports this pass and not an earlier one
int reset_attn_guards(mme_ctx* c, int layers, hipStream_t s);
