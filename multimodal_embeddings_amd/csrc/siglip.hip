// SigLIP ViT/16 @224 image towers (196 tokens, no class token): the kernel the tower adds beside the 196-token
// instantiation of the attention kernel (attention.hip), the tanh-GELU epilogues (gemm_epilogue.h) and rowops.hip's
// launch_embed_rows (tokens = 196, no class row) and launch_l2_rows_bf16.
//
//   map_pool         the attention of SiglipMultiheadAttentionPoolingHead: ONE learned query per head attends over the 196
//                    tokens of a crop.  kv bf16 [n * 196, 2 D] (K | V, the head's in_proj over post_layernorm(x)), q f32 [D]
//                    (probe . W_q^T + b_q, times dh^-0.5 log2 e: the same for every crop, prepared at load) -> a bf16 [n, D]:
//                      s_j = q_h . k_j (f32, d ascending), p_j = exp2(s_j - max_j s_j), a_h = (sum_j p_j v_j) / sum_j p_j,
//                    rounded once.  One wave per (crop, head), no LDS-DMA: the kernel reads 196 x 2 x 128 bytes per item once
//                    and is bound by that.  Scores: lane = key (four rounds of 64, the last one of 4), a key row of 128
//                    contiguous bytes per lane; p goes through 1 KiB of LDS per wave; P.V: lane = (row group g of 4, four
//                    head dims), so one instruction reads four whole 128-byte V rows, 49 steps, then two cross-lane adds
//                    ((g0 + g1) + (g2 + g3)).  Nothing at or past row 196 n is read.
// 64-bit offsets everywhere.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int T196 = 196;

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

}  // namespace

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
