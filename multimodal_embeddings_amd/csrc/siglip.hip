// SigLIP ViT/16 @224 image towers (196 tokens, no class token): the two kernels the tower adds beside the 196-token
// instantiation of the attention kernel (attention.hip) and the tanh-GELU epilogues (gemm_epilogue.h).
//
//   embed_rows_t196  the patch-embed GEMM runs with the f32 epilogue (acc [n * 196, D]); this kernel writes the residual
//                    stream with one rounding per value: x[b * 196 + p] = bf16((acc + bias) + pos[p]) -- the f32 order of
//                    the patch-embed epilogue of the 197-token path.
//   map_pool         the attention of SiglipMultiheadAttentionPoolingHead: ONE learned query per head attends over the 196
//                    tokens of a crop.  kv bf16 [n * 196, 2 D] (K | V, the head's in_proj over post_layernorm(x)), q f32 [D]
//                    (probe . W_q^T + b_q, times dh^-0.5 log2 e: the same for every crop, prepared at load) -> a bf16 [n, D]:
//                      s_j = q_h . k_j (f32, d ascending), p_j = exp2(s_j - max_j s_j), a_h = (sum_j p_j v_j) / sum_j p_j,
//                    rounded once.  One wave per (crop, head), no LDS-DMA: the kernel reads 196 x 2 x 128 bytes per item once
//                    and is bound by that.  Scores: lane = key (four rounds of 64, the last one of 4), a key row of 128
//                    contiguous bytes per lane; p goes through 1 KiB of LDS per wave; P.V: lane = (row group g of 4, four
//                    head dims), so one instruction reads four whole 128-byte V rows, 49 steps, then two cross-lane adds
//                    ((g0 + g1) + (g2 + g3)).  Nothing at or past row 196 n is read.
//   l2_rows_bf16     rowops.hip's l2_rows on bf16 rows (the head's output y is the residual stream's type): widened to f32,
//                    x / max(||x||, 1e-12) in l2_rows' arithmetic, to f32 and / or bf16.
// 64-bit offsets everywhere.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int T196 = 196;

// rowops.hip's RowShape: a row of D values over 64 lanes, NT accesses of V consecutive values per lane
template <int D> struct RowShape196 {
    static_assert(D == 384 || D == 768 || D == 1024, "row kernels: widths 384, 768 and 1024");
    static constexpr int V = (D % 256) == 0 ? 4 : 2;
    static constexpr int NT = D / (64 * V);
    typedef __attribute__((ext_vector_type(V))) __bf16 bvec;
    typedef __attribute__((ext_vector_type(V))) float fvec;
};

template <int D>
__global__ __launch_bounds__(256) void embed_rows_t196(const float* __restrict__ acc, const float* __restrict__ bias, const float* __restrict__ pos,
                                                       bf16_t* __restrict__ x, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int p = (int)(row % T196);
    typedef RowShape196<D> RS;
    constexpr int V = RS::V, NT = RS::NT;
    bf16_t* xr = x + row * D;
    const float* pr = pos + (int64_t)p * D;
    const float* ar = acc + row * D;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int c = k * 64 * V + lane * V;
        const typename RS::fvec pv = *(const typename RS::fvec*)(pr + c);
        const typename RS::fvec a = *(const typename RS::fvec*)(ar + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(bias + c);
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)((a[j] + bv[j]) + pv[j]);
        *(typename RS::bvec*)(xr + c) = o;
    }
}

template <int H>
__global__ __launch_bounds__(256) void map_pool(const bf16_t* __restrict__ kv, const float* __restrict__ q, bf16_t* __restrict__ out, int64_t items) {
    constexpr int D = H * VIT_DH;
    constexpr int64_t LD = 2 * D;  // elements per row of K | V
    __shared__ float p_s[4][256];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;  // wave-uniform
    if (item >= items) return;
    const int64_t b = item / H;
    const int h = (int)(item - b * H);
    const bf16_t* kb = kv + b * T196 * LD + h * VIT_DH;  // K row 0 of the item; V row 0 is D elements further
    const float* qh = q + h * VIT_DH;
    // scores of keys lane, lane + 64, lane + 128, lane + 192 (< 196)
    float sc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        float s = 0.f;
        if (j < T196) {
            const bf16_t* kr = kb + (int64_t)j * LD;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const bf16x8 k8 = *(const bf16x8*)(kr + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qh[c * 8 + e], (float)k8[e], s);
            }
        }
        sc[i] = s;
    }
    float mx = fmaxf(fmaxf(sc[0], sc[1]), sc[2]);  // keys 0..191 exist in every lane
    if (lane < T196 - 192) mx = fmaxf(mx, sc[3]);
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        const float p = j < T196 ? __builtin_amdgcn_exp2f(sc[i] - mx) : 0.f;
        p_s[wave][j] = p;
        sum += p;
    }
    sum = wave_sum(sum);  // >= 1: the maximum contributes exp2(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's own LDS writes before its reads below
    // P.V: lane = (g, c): rows g, g + 4, ... (49 of them), head dims 4 c .. 4 c + 3
    const int g = lane >> 4, c4 = (lane & 15) * 4;
    const bf16_t* vb = kb + D + c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 7
    for (int j0 = 0; j0 < T196; j0 += 4) {
        const int j = j0 + g;
        const float p = p_s[wave][j];
        const bf16x4 v = *(const bf16x4*)(vb + (int64_t)j * LD);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(p, (float)v[e], acc[e]);
    }
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float a = acc[e];
        a += __shfl_xor(a, 16, 64);  // g0 + g1, g2 + g3
        a += __shfl_xor(a, 32, 64);
        o[e] = (bf16_t)(a / sum);
    }
    if (g == 0) *(bf16x4*)(out + b * D + h * VIT_DH + c4) = o;
}

__global__ __launch_bounds__(256) void l2_rows_bf16(const bf16_t* __restrict__ x, int64_t rows, int p, float* __restrict__ y_f32,
                                                    bf16_t* __restrict__ y_bf16) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* xr = x + row * p;
    f32x4 v[4];
    float n2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < p) {
            const bf16x4 b = *(const bf16x4*)(xr + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = (float)b[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) n2 += v[k][j] * v[k][j];
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        if (c >= p) continue;
        f32x4 o;
        bf16x4 ob;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = v[k][j] * inv;
            ob[j] = (bf16_t)o[j];
        }
        if (y_f32) *(f32x4*)(y_f32 + row * p + c) = o;
        if (y_bf16) *(bf16x4*)(y_bf16 + row * p + c) = ob;
    }
}

}  // namespace

hipError_t launch_embed_rows_t196(const float* acc, const float* bias, const float* pos, void* x, int n, int d, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t rows = (int64_t)n * T196;
    const dim3 grid((unsigned)((rows + 3) / 4));
    switch (d) {
        case 384: hipLaunchKernelGGL(embed_rows_t196<384>, grid, dim3(256), 0, s, acc, bias, pos, (bf16_t*)x, rows); break;
        case 768: hipLaunchKernelGGL(embed_rows_t196<768>, grid, dim3(256), 0, s, acc, bias, pos, (bf16_t*)x, rows); break;
        default: hipLaunchKernelGGL(embed_rows_t196<1024>, grid, dim3(256), 0, s, acc, bias, pos, (bf16_t*)x, rows); break;
    }
    return hipGetLastError();
}

hipError_t launch_map_pool(const void* kv, const float* q, void* out, int n, int heads, hipStream_t s) {
    if (heads != 6 && heads != 12 && heads != 16) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t items = (int64_t)n * heads;
    const dim3 grid((unsigned)((items + 3) / 4));
    switch (heads) {
        case 6: hipLaunchKernelGGL(map_pool<6>, grid, dim3(256), 0, s, (const bf16_t*)kv, q, (bf16_t*)out, items); break;
        case 12: hipLaunchKernelGGL(map_pool<12>, grid, dim3(256), 0, s, (const bf16_t*)kv, q, (bf16_t*)out, items); break;
        default: hipLaunchKernelGGL(map_pool<16>, grid, dim3(256), 0, s, (const bf16_t*)kv, q, (bf16_t*)out, items); break;
    }
    return hipGetLastError();
}

hipError_t launch_l2_rows_bf16(const void* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    if (p < 64 || (p % 64) != 0 || p > 1024) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(l2_rows_bf16, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const bf16_t*)x, rows, p, y_f32, (bf16_t*)y_bf16);
    return hipGetLastError();
}
