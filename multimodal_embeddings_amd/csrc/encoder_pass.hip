// The launch sequence of one pre-LN transformer block, written once for every tower (encoder_pass.h).
#include "encoder_pass.h"

int EncoderPass::gemm(int epilogue, const GemmArgs& g) {
    Timed t(c, s, KC_GEMM);
    HIP_TRY(c, launch_gemm(epilogue, g, s, c->gemm_variant));
    return MME_OK;
}

int EncoderPass::stats_from_x(const void* xr, int64_t row0, int64_t rows) {
    Timed t(c, s, KC_LN);
    HIP_TRY(c, launch_ln_stats_canonical(xr, row0, rows, D, eps, stats, s));
    return MME_OK;
}

int EncoderPass::stats_after(const GemmArgs& producer, int64_t rows) {
    const int64_t interior = planes ? gemm_interior_rows(EPI_BIAS_RES_STATS, producer, c->gemm_variant) : 0;
    if (interior == 0) return stats_from_x(producer.out, 0, rows);
    {
        Timed t(c, s, KC_LN);
        HIP_TRY(c, launch_ln_finish(lnpart, lnpart_rows, interior, D, eps, stats, s));
    }
    return interior < rows ? stats_from_x(producer.out, interior, rows) : MME_OK;
}

int EncoderPass::residual(const void* a, const bf16_t* w, const float* bias, int K, int rows, void* xr, bool stats_next) {
    GemmArgs g{};
    g.A = a; g.W = w; g.M = rows; g.N = D; g.K = K;
    g.bias = bias; g.out = xr; g.res = xr; g.ldo = D;
    if (lnpart) {
        g.ln_part = lnpart;
        g.ln_part_rows = lnpart_rows;
    }
    g.reverse_m = next_dir();
    int r;
    if ((r = gemm(planes && stats_next ? EPI_BIAS_RES_STATS : EPI_BIAS_RES, g))) return r;
    return stats_next ? stats_after(g, rows) : MME_OK;
}

int EncoderPass::qkv_ln(const BlockW& w, int rows, int N) {
    GemmArgs g{};
    g.A = x; g.W = w.qkv_wf; g.M = rows; g.N = N; g.K = D;
    g.bias = w.qkv_bf; g.colsum = w.qkv_cs; g.ln_stats = stats; g.out = qkv; g.ldo = N;
    g.reverse_m = next_dir();
    return gemm(EPI_LN_BIAS, g);
}

int EncoderPass::fc1_ln(const BlockW& w, int rows, const void* xr) {
    GemmArgs g{};
    g.A = xr; g.W = w.fc1_wf; g.M = rows; g.N = F; g.K = D;
    g.bias = w.fc1_bf; g.colsum = w.fc1_cs; g.ln_stats = stats; g.out = mlp; g.ldo = F;
    g.reverse_m = next_dir();
    return gemm(act == 2 ? EPI_LN_BIAS_TGELU : act ? EPI_LN_BIAS_QGELU : EPI_LN_BIAS_GELU, g);
}

int EncoderPass::after_attention(const BlockW& w, int rows, const void* a, void* xr, bool stats_next) {
    int r;
    if ((r = residual(a, w.o_w, w.o_b, D, rows, xr, true))) return r;
    if ((r = fc1_ln(w, rows, xr))) return r;
    return residual(mlp, w.fc2_w, w.fc2_b, F, rows, xr, stats_next);
}

int EncoderPass::layernorm(const void* xr, const float* gamma, const float* beta, int rows) {
    Timed t(c, s, KC_LN);
    HIP_TRY(c, launch_layernorm(xr, gamma, beta, hbuf, rows, D, eps, s));
    return MME_OK;
}

int EncoderPass::first_half(const LayerDev& L, const float* gamma, const float* beta, int rows, int N) {
    if (!unfolded()) return qkv_ln(L.w, rows, N);
    int r;
    if ((r = layernorm(x, gamma, beta, rows))) return r;
    GemmArgs g{};
    g.A = hbuf; g.W = L.qkv_w; g.M = rows; g.N = N; g.K = D;
    g.bias = L.qkv_b; g.out = qkv; g.ldo = N;
    g.reverse_m = next_dir();
    return gemm(EPI_BIAS, g);
}

int EncoderPass::second_half(const LayerDev& L, int rows, const void* a, void* xr, bool stats_next) {
    if (!unfolded()) return after_attention(L.w, rows, a, xr, stats_next);
    int r;
    if ((r = residual(a, L.w.o_w, L.w.o_b, D, rows, xr, false))) return r;
    if ((r = layernorm(xr, L.ln2_g, L.ln2_b, rows))) return r;
    GemmArgs g{};
    g.A = hbuf; g.W = L.fc1_w; g.M = rows; g.N = F; g.K = D;
    g.bias = L.fc1_b; g.out = mlp; g.ldo = F;
    g.reverse_m = next_dir();
    if ((r = gemm(act == 2 ? EPI_BIAS_TGELU : act ? EPI_BIAS_QGELU : EPI_BIAS_GELU, g))) return r;
    return residual(mlp, L.w.fc2_w, L.w.fc2_b, F, rows, xr, false);
}

int reset_attn_guards(mme_ctx* c, int layers, hipStream_t s) {
    const size_t bytes = (size_t)(layers > VIT_MAX_L ? layers : VIT_MAX_L) * sizeof(int);
    int r;
    if ((r = ensure(c, c->attn_guard, bytes))) return r;
    HIP_TRY(c, hipMemsetAsync(c->attn_guard.p, 0, bytes, s));
    return MME_OK;
}
