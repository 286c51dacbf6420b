// Mean pooling over the patch tokens a crop covers: pool = "mean" and "cls+mean" of the ViT and DINOv2 towers.
//
// For crop b with covered grid (R, C) on a g x g patch grid, y_t = the final LayerNorm of residual row b * tokens + t (ln_row's
// arithmetic, K8's), S = {first + r * g + c : r < R, c < C} in row-major order j = r * C + c, P = R * C:
//     m = (sum_{t in S} y_t) / P;   mean: m / max(||m||, 1e-12);   cls+mean: [y_0 | m] / max(||[y_0 | m]||, 1e-12).
// One workgroup of four waves per crop.  The summation order is a fixed function of (R, C):
//     wave w sums the covered tokens j = w, w + 4, w + 8, ... in ascending j, starting FROM its first row (not from zero);
//     the partial sums meet in LDS and wave 0 adds those that exist in ascending w: ((p0 + p1) + p2) + p3;
//     the sum is multiplied by the f32 value 1.0f / P.
// So (1, 1) is K8's row for pool_token = first bit for bit (p0 * 1.0f).  A wave issues the raw bf16 loads of POOL_U rows, 3 or 4
// per lane and row, unconditionally (a row past the last one re-reads the first) and widens and normalises them afterwards:
// POOL_U x 3 or 4 loads per lane in flight instead of a chain of up to 64 rows.
#include "common.h"
#include "kernels.h"
#include "row_kernels.h"

namespace {

constexpr int POOL_WAVES = 4;  // the workgroup of ROW_KERNEL_BY_WIDTH
constexpr int POOL_U = 8;      // rows of one wave in flight (6 or 8 VGPRs of raw bf16 each)

template <int D, bool CLS>
__device__ __forceinline__ void pool_mean_body(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                               const int32_t* __restrict__ grids, int tokens, int g, int first, float eps,
                                               float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    constexpr int NV = D / 64;
    __shared__ float part[POOL_WAVES - 1][NV][64];  // the partial sums of waves 1..3, register-major: lane-contiguous, no bank conflict
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    // the launchers' callers validate the grids; the clamp keeps a bad device table inside the crop's own rows
    int R = g, C = g;
    if (grids) {
        R = min(max(grids[2 * b], 1), g);
        C = min(max(grids[2 * b + 1], 1), g);
    }
    const int P = R * C;
    const bf16_t* xb = x + b * tokens * D;  // 64-bit: 65 536 crops x 257 x 1024 values
    float acc[NV] = {};
    bool have = false;  // the first row of a wave is assigned, not added to zero: -0 stays -0 and (1, 1) is K8's row
    typedef RowShape<D> RS;
    int r = wave / C, c = wave - r * C;  // (row, column) of the wave's next covered token: the only division, then steps of POOL_WAVES
    for (int j0 = wave; j0 < P; j0 += POOL_WAVES * POOL_U) {
        // every load of the batch is issued, unconditionally, before the first value is used: a row past the crop's last one
        // re-reads the first covered row (a valid address, the value dropped), so no load waits behind a branch
        typename RS::bvec raw[POOL_U][RS::NT];
#pragma unroll
        for (int u = 0; u < POOL_U; ++u) {
            const int tok = j0 + u * POOL_WAVES < P ? first + r * g + c : first;
            row_load_raw<D>(xb + (int64_t)tok * D, lane, raw[u]);
            c += POOL_WAVES;
            while (c >= C) {  // at most POOL_WAVES steps (C = 1)
                c -= C;
                ++r;
            }
        }
#pragma unroll
        for (int u = 0; u < POOL_U; ++u) {
            if (j0 + u * POOL_WAVES < P) {  // wave-uniform
                float v[NV];
                row_widen<D>(raw[u], v);
                ln_apply<D>(gamma, beta, eps, lane, v);
                if (have) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) acc[k] += v[k];
                } else {
#pragma unroll
                    for (int k = 0; k < NV; ++k) acc[k] = v[k];
                    have = true;
                }
            }
        }
    }
    if (wave > 0 && have) {
#pragma unroll
        for (int k = 0; k < NV; ++k) part[wave - 1][k][lane] = acc[k];
    }
    __syncthreads();
    if (wave != 0) return;
    const int nw = P < POOL_WAVES ? P : POOL_WAVES;  // waves that held a row
    for (int w = 1; w < nw; ++w) {
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += part[w - 1][k][lane];
    }
    const float invP = 1.0f / (float)P;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] *= invP;
    if (!CLS) {
        row_l2_store<D>(acc, lane, emb_f32, emb_bf16, b * D);
        return;
    }
    // [y_0 | m]: one norm over the 2 D values, the class half first
    float y0[NV];
    ln_row<D>(xb, gamma, beta, eps, lane, y0);
    const float inv = l2_inverse(wave_sum(row_sumsq<D>(y0) + row_sumsq<D>(acc)));
    row_scale_store<D>(y0, inv, lane, emb_f32, emb_bf16, b * 2 * D);
    row_scale_store<D>(acc, inv, lane, emb_f32, emb_bf16, b * 2 * D + D);
}

template <int D>
__global__ __launch_bounds__(256) void pool_mean_ln_l2(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const int32_t* __restrict__ grids, int tokens, int g, int first, float eps,
                                                       float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    pool_mean_body<D, false>(x, gamma, beta, grids, tokens, g, first, eps, emb_f32, emb_bf16);
}
template <int D>
__global__ __launch_bounds__(256) void pool_cls_mean_ln_l2(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const int32_t* __restrict__ grids, int tokens, int g, int first, float eps,
                                                           float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    pool_mean_body<D, true>(x, gamma, beta, grids, tokens, g, first, eps, emb_f32, emb_bf16);
}

}  // namespace

hipError_t launch_pool_mean(const void* x, const float* gamma, const float* beta, const int32_t* grids, int B, int tokens, int g, int first,
                            bool cls_mean, int d, float eps, float* emb_f32, void* emb_bf16, hipStream_t s) {
    if (!vit_width_built(d) || g < 1 || g > 16 || (first != 0 && first != 1) || tokens != first + g * g || (cls_mean && first != 1))
        return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    if (cls_mean) {
        ROW_KERNEL_BY_WIDTH(d, pool_cls_mean_ln_l2, dim3((unsigned)B), s, (const bf16_t*)x, gamma, beta, grids, tokens, g, first, eps, emb_f32,
                            (bf16_t*)emb_bf16)
    } else {
        ROW_KERNEL_BY_WIDTH(d, pool_mean_ln_l2, dim3((unsigned)B), s, (const bf16_t*)x, gamma, beta, grids, tokens, g, first, eps, emb_f32,
                            (bf16_t*)emb_bf16)
    }
    return hipGetLastError();
}
