// ViT/32 @224 (7 x 7 patches of 32 x 32, 50 tokens): the kernels the second image geometry adds beside its attention
// kernel (attention_short.hip).  K1, the GEMMs and the 197-token row kernels are untouched and compiled as before.
//
//   retile_patches_p32  K1 writes the bf16 patch-16 matrix [n * 196, 768] under both resize rules and every emitter form;
//                       this kernel permutes it to the patch-32 matrix [n * 49, 3072] in conv order (c, ky, kx).  A
//                       32 x 32 patch is four 16 x 16 patches, and a run of 16 kx values is contiguous on both sides:
//                         destination row b * 49 + PY * 7 + PX,                column c * 1024 + KY * 32 + KX
//                         source row      b * 196 + (2 PY + KY / 16) * 14 + 2 PX + KX / 16, column c * 256 + (KY % 16) * 16 + KX % 16
//                       A pure copy in 16-byte pieces (half a run per thread, consecutive lanes write consecutive bytes).
//   embed_rows_t50      the patch-embed GEMM runs with the f32 epilogue (acc [n * 49, D]); this kernel writes the residual
//                       stream with one rounding per value: x[b * 50 + 1 + p] = bf16((acc + bias) + pos[1 + p]) -- the f32
//                       order of the patch-embed epilogue of the 197-token path -- and x[b * 50] = bf16(cls + pos[0]).
//   pool_ln_rows_t50 / pool_ln_l2_t50   rowops.hip's pooling kernels on row b * 50 + tok.
// One 64-lane wave per row in the row kernels, 64-bit offsets everywhere.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int T50 = 50, NP49 = 49, GRID7 = 7;
constexpr int P32_DIM = 3 * 32 * 32;            // 3072
constexpr int64_t PIECES_PER_CROP = NP49 * P32_DIM / 8;  // 16-byte pieces of one crop: 18 816

// rowops.hip's RowShape: a row of D values over 64 lanes, NT accesses of V consecutive values per lane
template <int D> struct RowShape50 {
    static_assert(D == 384 || D == 768 || D == 1024, "row kernels: widths 384, 768 and 1024");
    static constexpr int V = (D % 256) == 0 ? 4 : 2;
    static constexpr int NT = D / (64 * V);
    static constexpr int PER_LANE = D / 64;
    typedef __attribute__((ext_vector_type(V))) __bf16 bvec;
    typedef __attribute__((ext_vector_type(V))) float fvec;
};

__global__ __launch_bounds__(256) void retile_patches_p32(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int64_t pieces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pieces) return;
    const int64_t b = i / PIECES_PER_CROP;
    const int rem = (int)(i - b * PIECES_PER_CROP);  // piece of the crop, in destination order
    const int P = rem / (P32_DIM / 8), piece = rem - P * (P32_DIM / 8);   // 384 pieces per destination row
    const int c = piece >> 7, within = piece & 127;                      // 128 pieces per channel
    const int KY = within >> 2, kxq = within & 3;                        // four pieces (KX = 8 kxq ..) per row of the patch
    const int PY = P / GRID7, PX = P - PY * GRID7;
    const int64_t srow = b * 196 + (2 * PY + (KY >> 4)) * 14 + 2 * PX + (kxq >> 1);
    const int scol = c * 256 + (KY & 15) * 16 + (kxq & 1) * 8;
    const uint4 v = *(const uint4*)(src + srow * 768 + scol);
    *(uint4*)(dst + i * 8) = v;
}

template <int D>
__global__ __launch_bounds__(256) void embed_rows_t50(const float* __restrict__ acc, const float* __restrict__ bias, const float* __restrict__ pos,
                                                      const float* __restrict__ cls, bf16_t* __restrict__ x, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / T50;
    const int t = (int)(row - b * T50);
    typedef RowShape50<D> RS;
    constexpr int V = RS::V, NT = RS::NT;
    bf16_t* xr = x + row * D;
    const float* pr = pos + (int64_t)t * D;
    const float* ar = acc + (b * NP49 + (t ? t - 1 : 0)) * D;  // read for t >= 1 only
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int c = k * 64 * V + lane * V;
        const typename RS::fvec p = *(const typename RS::fvec*)(pr + c);
        typename RS::bvec o;
        if (t == 0) {
            const typename RS::fvec a = *(const typename RS::fvec*)(cls + c);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = (bf16_t)(a[j] + p[j]);
        } else {
            const typename RS::fvec a = *(const typename RS::fvec*)(ar + c);
            const typename RS::fvec bv = *(const typename RS::fvec*)(bias + c);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = (bf16_t)((a[j] + bv[j]) + p[j]);
        }
        *(typename RS::bvec*)(xr + c) = o;
    }
}

// LayerNorm of row b * 50 + tok in the two-pass f32 arithmetic of rowops.hip; v[] leaves normalised, scaled and shifted
template <int D>
__device__ __forceinline__ void ln_row_t50(const bf16_t* __restrict__ xr, const float* __restrict__ gamma, const float* __restrict__ beta,
                                           float eps, int lane, float (&v)[D / 64]) {
    typedef RowShape50<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const typename RS::bvec p = *(const typename RS::bvec*)(xr + t * 64 * V + lane * V);
#pragma unroll
        for (int j = 0; j < V; ++j) v[t * V + j] = (float)p[j];
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) s += v[j];
    const float mean = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        v[j] -= mean;
        q += v[j] * v[j];
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        const typename RS::fvec gv = *(const typename RS::fvec*)(gamma + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(beta + c);
#pragma unroll
        for (int j = 0; j < V; ++j) v[t * V + j] = v[t * V + j] * rstd * gv[j] + bv[j];
    }
}

template <int D>
__global__ __launch_bounds__(256) void pool_ln_rows_t50(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int B, int tok, float eps, bf16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    typedef RowShape50<D> RS;
    constexpr int V = RS::V, NT = RS::NT;
    float v[RS::PER_LANE];
    ln_row_t50<D>(x + ((int64_t)b * T50 + tok) * D, gamma, beta, eps, lane, v);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)v[t * V + j];
        *(typename RS::bvec*)(y + (int64_t)b * D + c) = o;
    }
}

template <int D>
__global__ __launch_bounds__(256) void pool_ln_l2_t50(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int B, int tok, float eps, float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    typedef RowShape50<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
    ln_row_t50<D>(x + ((int64_t)b * T50 + tok) * D, gamma, beta, eps, lane, v);
    float n2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) n2 += v[j] * v[j];
    // torch.nn.functional.normalize: x / max(||x||_2, 1e-12)
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), 1e-12f);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        typename RS::fvec o;
        typename RS::bvec ob;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            o[j] = v[t * V + j] * inv;
            ob[j] = (bf16_t)o[j];
        }
        if (emb_f32) *(typename RS::fvec*)(emb_f32 + (int64_t)b * D + c) = o;
        if (emb_bf16) *(typename RS::bvec*)(emb_bf16 + (int64_t)b * D + c) = ob;
    }
}

}  // namespace

#define ROW_KERNEL_BY_WIDTH_T50(d, kernel, grid, s, ...)                                                      \
    switch (d) {                                                                                              \
        case 384: hipLaunchKernelGGL(kernel<384>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 768: hipLaunchKernelGGL(kernel<768>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 1024: hipLaunchKernelGGL(kernel<1024>, grid, dim3(256), 0, s, __VA_ARGS__); break;               \
        default: return hipErrorInvalidValue;                                                                 \
    }

hipError_t launch_retile_p32(const void* patches16, void* patches32, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t pieces = (int64_t)n * PIECES_PER_CROP, blocks = (pieces + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(retile_patches_p32, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)patches16, (bf16_t*)patches32, pieces);
    return hipGetLastError();
}

hipError_t launch_embed_rows_t50(const float* acc, const float* bias, const float* pos, const float* cls, void* x, int n, int d, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t rows = (int64_t)n * T50;
    ROW_KERNEL_BY_WIDTH_T50(d, embed_rows_t50, dim3((unsigned)((rows + 3) / 4)), s, acc, bias, pos, cls, (bf16_t*)x, rows)
    return hipGetLastError();
}

hipError_t launch_pool_ln_t50(const void* x, const float* gamma, const float* beta, int B, int tok, int d, float eps, void* y, hipStream_t s) {
    if (!vit_width_built(d) || tok < 0 || tok >= T50) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH_T50(d, pool_ln_rows_t50, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tok, eps, (bf16_t*)y)
    return hipGetLastError();
}

hipError_t launch_pool_t50(const void* x, const float* gamma, const float* beta, int B, int tok, int d, float eps, float* emb_f32, void* emb_bf16,
                           hipStream_t s) {
    if (!vit_width_built(d) || tok < 0 || tok >= T50) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH_T50(d, pool_ln_l2_t50, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tok, eps, emb_f32, (bf16_t*)emb_bf16)
    return hipGetLastError();
}
