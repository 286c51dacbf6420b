// Row kernels of the CLIP text tower (transformers models/clip/modeling_clip.py, CLIPTextEmbeddings and the pooling of
// CLIPTextTransformer.forward): the token rows that open the pass and the LayerNorm of the EOS rows that closes it.
// One 64-lane wave owns one row of D values, D = 512, 768 or 1024 (8, 12, 16 heads of 64).  The sequence length is 77
// (TXT_T, CLIP) or 64 (TXT_T64, the SigLIP text tower: transformers models/siglip/modeling_siglip.py, SiglipTextEmbeddings
// and SiglipTextTransformer's last_hidden_state[:, -1, :] -- eos_pool_ln_rows with every position 63; the head's bias and
// the L2 step are rowops.hip's launch_bias_l2_rows).
// siglip_scores is SiglipModel.forward's sigmoid(exp(logit_scale) cos + logit_bias) on a cosine block.
#include "common.h"
#include "kernels.h"
#include "row_kernels.h"

namespace {

// x[b * T + t] = bf16(f32(tok[ids[b, t]]) + pos[t]): one f32 add, one rounding to nearest even.  64-bit offsets: a
// 65536 x 1024 table holds 2^26 values (262144 x 1024: 2^28), n * 77 * D passes 2^31 at n = 27 236 (D = 1024).
template <int T>
__global__ __launch_bounds__(256) void token_rows(const bf16_t* __restrict__ tok, const float* __restrict__ pos, const int32_t* __restrict__ ids,
                                                  bf16_t* __restrict__ x, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = (int)(row % T);
    const bf16_t* tr = tok + (int64_t)ids[row] * D;
    const float* pr = pos + (int64_t)t * D;
    bf16_t* xr = x + row * D;
    for (int c = lane * 4; c < D; c += 256) {
        const bf16x4 e = *(const bf16x4*)(tr + c);
        const f32x4 p = *(const f32x4*)(pr + c);
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16_t)((float)e[j] + p[j]);
        *(bf16x4*)(xr + c) = o;
    }
}

// final_layer_norm of row b * tokens + eos_pos[b], the LayerNorm of rowops.hip's pool_ln_rows, rounded to bf16 [n, D]
// for the projection GEMM and / or left in f32 [n, D] (a tower without text_projection: the L2 step reads that).
template <int D>
__global__ __launch_bounds__(256) void eos_pool_ln_rows(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const int32_t* __restrict__ eos_pos, int n, int tokens, float eps, bf16_t* __restrict__ y,
                                                        float* __restrict__ yf) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    typedef RowShape<D> RS;
    float v[D / 64];
    ln_row<D>(x + ((int64_t)b * tokens + eos_pos[b]) * D, gamma, beta, eps, lane, v);
    if (y) row_store_bf16<D>(y + (int64_t)b * D, lane, v);
    if (yf) {
#pragma unroll
        for (int t = 0; t < RS::NT; ++t) {
            typename RS::fvec o;
#pragma unroll
            for (int j = 0; j < RS::V; ++j) o[j] = v[t * RS::V + j];
            *(typename RS::fvec*)(yf + (int64_t)b * D + t * 64 * RS::V + lane * RS::V) = o;
        }
    }
}

// p = 1 / (1 + exp(-(c * scale + bias))), scale = exp(logit_scale) formed once on the host: one multiply, one add, one exp,
// one add and one division in f32, in place when out == cos.  Finite for every finite c: z -> -inf gives exp = +inf and
// p = 0, z -> +inf gives exp = 0 and p = 1; there is no inf - inf and no 0 * inf on the way.
__global__ __launch_bounds__(256) void siglip_scores(const float* __restrict__ cos, float* __restrict__ out, int64_t count, float scale, float bias) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const float z = cos[i] * scale + bias;
        out[i] = 1.0f / (1.0f + expf(-z));
    }
}

}  // namespace

constexpr bool text_layout(const TokenLayout& L) { return !L.image(); }  // the layouts token_rows is instantiated for:
static_assert(count_layouts(text_layout) == 2 && text_layout(*find_layout(TXT_T)) && text_layout(*find_layout(TXT_T64)), "token_rows: one instantiation per text layout");

hipError_t launch_text_token_rows(const void* tok, const float* pos, const int32_t* ids, void* x, int n, int d, hipStream_t s, int tokens) {
    const TokenLayout* L = find_layout(tokens);
    if (!text_width_built(d) || !L || !text_layout(*L)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t rows = (int64_t)n * tokens;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (tokens == TXT_T) hipLaunchKernelGGL(token_rows<TXT_T>, grid, dim3(256), 0, s, (const bf16_t*)tok, pos, ids, (bf16_t*)x, rows, d);
    else hipLaunchKernelGGL(token_rows<TXT_T64>, grid, dim3(256), 0, s, (const bf16_t*)tok, pos, ids, (bf16_t*)x, rows, d);
    return hipGetLastError();
}

hipError_t launch_text_eos_pool_ln(const void* x, const float* gamma, const float* beta, const int32_t* eos_pos, int n, int d, float eps, void* y,
                                   float* y_f32, hipStream_t s, int tokens) {
    const TokenLayout* L = find_layout(tokens);
    if (!text_width_built(d) || !L || !text_layout(*L) || !L->pooled) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, eos_pool_ln_rows, dim3((n + 3) / 4), s, (const bf16_t*)x, gamma, beta, eos_pos, n, tokens, eps, (bf16_t*)y, y_f32)
    return hipGetLastError();
}

hipError_t launch_siglip_scores(const float* cos, float* out, int64_t count, float scale, float bias, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(siglip_scores, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, cos, out, count, scale, bias);
    return hipGetLastError();
}
