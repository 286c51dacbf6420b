// Row-wise HBM-bound kernels of the ViT forward: LayerNorm (K3), [CLS] row initialisation,
// and final-LayerNorm + pooling + L2 normalisation (K8).
//
// One 64-lane wave owns one D-wide row: 3 x 8-byte (bf16x4) loads per lane at D = 768, statistics
// in f32 registers, two wave reductions (mean, then centred variance -- the same two-pass
// form torch's LayerNorm uses, transformers modeling_vit.py:261-262,348), 8-byte stores.
// Instantiated per supported width (RowShape): 768 = 3 x 4 values per lane (the ViT-B/16 code as it always was),
// 1024 = 4 x 4, 384 = 3 x 2 (4-byte accesses: 384 is no multiple of the 256 values a wave covers with 8-byte ones).
#include "common.h"
#include "gemm_epilogue.h"
#include "kernels.h"

namespace {

// a row of D values over 64 lanes: NT accesses of V consecutive values per lane, access t at column t * 64 V + lane * V
template <int D> struct RowShape {
    static_assert(D == 384 || D == 768 || D == 1024, "row kernels: widths 384, 768 and 1024");
    static constexpr int V = (D % 256) == 0 ? 4 : 2;
    static constexpr int NT = D / (64 * V);
    static constexpr int PER_LANE = D / 64;
    typedef __attribute__((ext_vector_type(V))) __bf16 bvec;
    typedef __attribute__((ext_vector_type(V))) float fvec;
};

template <int D>
__global__ __launch_bounds__(256) void layernorm_rows(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                      int64_t rows, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* xr = x + row * D;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
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
    bf16_t* yr = y + row * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        const typename RS::fvec gv = *(const typename RS::fvec*)(gamma + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(beta + c);
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)(v[t * V + j] * rstd * gv[j] + bv[j]);
        *(typename RS::bvec*)(yr + c) = o;
    }
}

// LayerNorm statistics only (mean, rstd) of bf16 rows of D: the normalisation itself is
// folded into the GEMM that consumes the row (EPI_LN_*), so the residual stream is read once
// and nothing is written back but 8 bytes per row.  Same two-pass f32 arithmetic as
// layernorm_rows, so the folded path sees the statistics LayerNorm would have used.
template <int D>
__global__ __launch_bounds__(256) void ln_stats_rows(const bf16_t* __restrict__ x, int64_t rows, float eps, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* xr = x + row * D;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
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
        const float d = v[j] - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
    if (lane == 0) *(float2*)(stats + 2 * row) = make_float2(mean, rstd);
}

// The same statistics in the canonical order of gemm_epilogue.h (ln_accumulate / ln_finish_row): one wave per
// row, lane = (slice, column group g) for up to two rounds of 16 slices; 48 of the 64 lanes carry data at d = 768.  Used wherever no
// EPI_BIAS_RES_STATS epilogue produced the partial sums: the first LayerNorm of a pass, small problems that run
// the 128 x 128 kernel, the rows of a ragged last row tile.
__global__ __launch_bounds__(256) void ln_stats_canonical_rows(const bf16_t* __restrict__ x, int64_t row0, int64_t row1, int d, float eps,
                                                               float* __restrict__ stats, int64_t stride) {
    const int lane = threadIdx.x & 63;
    const int64_t row = row0 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * stride;  // rows row0, row0 + stride, ... < row1
    if (row >= row1) return;
    const int slice = lane >> 2, grp = lane & 3, nslice = d >> 6;  // a lane serves slices `slice` and `slice + 16` (d <= 2048)
    float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int sl = slice + 16 * h;
        if (sl < nslice) {
            const bf16_t* xr = x + row * d + sl * 64 + grp * 4;
            uint2 pk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pk[j] = *(const uint2*)(xr + j * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) ln_accumulate(pk[j], s[h], q[h]);
        }
        s[h] += __shfl_xor(s[h], 1, 64);  // g0 + g1 | g2 + g3
        q[h] += __shfl_xor(q[h], 1, 64);
        s[h] += __shfl_xor(s[h], 2, 64);  // (g0 + g1) + (g2 + g3)
        q[h] += __shfl_xor(q[h], 2, 64);
    }
    double S = 0.0, Q = 0.0;
    for (int k = 0; k < nslice; ++k) {
        S += (double)__shfl(k < 16 ? s[0] : s[1], 4 * (k & 15), 64);
        Q += (double)__shfl(k < 16 ? q[0] : q[1], 4 * (k & 15), 64);
    }
    if (lane == 0) *(float2*)(stats + 2 * row) = ln_finish_row(S, Q, d, eps);
}

// rows [0, rows): the partial planes of an EPI_BIAS_RES_STATS GEMM -> (mean, rstd); one thread per row, the
// plane reads are coalesced over the rows
__global__ __launch_bounds__(256) void ln_finish_rows(const float* __restrict__ part, int64_t part_rows, int64_t rows, int d, float eps,
                                                      float* __restrict__ stats) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int nslice = d >> 6;
    double S = 0.0, Q = 0.0;
    for (int k = 0; k < nslice; ++k) {
        S += (double)part[(int64_t)k * part_rows + row];
        Q += (double)part[(int64_t)(nslice + k) * part_rows + row];
    }
    *(float2*)(stats + 2 * row) = ln_finish_row(S, Q, d, eps);
}

template <int D>
__global__ __launch_bounds__(256) void cls_rows(bf16_t* __restrict__ x, const float* __restrict__ cls,
                                                const float* __restrict__ pos, int B) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT;
    bf16_t* xr = x + (int64_t)b * VIT_T * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        const typename RS::fvec a = *(const typename RS::fvec*)(cls + c);
        const typename RS::fvec p = *(const typename RS::fvec*)(pos + c);
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)(a[j] + p[j]);
        *(typename RS::bvec*)(xr + c) = o;
    }
}

// K8: restates last_pooling (deprecated_package/embedder.py:17-34) for one fixed token
// index per sequence, after the final LayerNorm of that row only (the other 196 rows of
// the last hidden state are never read by the reference's pooling).
template <int D>
__global__ __launch_bounds__(256) void pool_ln_l2(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, int B, int tok, float eps,
                                                  float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16_t* xr = x + ((int64_t)b * VIT_T + tok) * D;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
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
    float n2 = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        const typename RS::fvec gv = *(const typename RS::fvec*)(gamma + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(beta + c);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            v[t * V + j] = v[t * V + j] * rstd * gv[j] + bv[j];
            n2 += v[t * V + j] * v[t * V + j];
        }
    }
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

// f32 rows of any width d (d % 4 == 0) -> L2-normalised bf16 rows (one wave per row).  The
// reference hands vectors around as Python float lists (embedder.py:132); this is the way
// such vectors enter the bf16 cosine kernel, with the same normalisation as last_pooling.
__global__ __launch_bounds__(256) void normalise_rows_f32(const float* __restrict__ x, int64_t rows, int d, bf16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * d;
    float n2 = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        n2 += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), 1e-12f);
    bf16_t* yr = y + row * d;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16_t)(v[j] * inv);
        *(bf16x4*)(yr + c) = o;
    }
}

// CLIP's pre_layrnorm (transformers modeling_clip.py, CLIPVisionTransformer.forward: hidden_states = self.pre_layrnorm(
// hidden_states) before the encoder): LayerNorm(gamma, beta) of every token row IN PLACE, the two-pass f32 arithmetic of
// layernorm_rows, and in the same launch the (mean, rstd) of the ROUNDED row in the canonical order of gemm_epilogue.h --
// what ln_stats_canonical_rows would find in x afterwards, bit for bit -- so that the first folded LayerNorm of the pass
// needs no further pass over x.  The rounded row goes through the wave's own 2 D bytes of LDS to change from the row
// layout (RowShape) to the canonical one (lane = slice, column group).
template <int D>
__global__ __launch_bounds__(256) void pre_ln_rows(bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   int64_t rows, float eps, float* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) bf16_t rowbuf[4][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;  // wave-uniform: no workgroup barrier below
    bf16_t* xr = x + row * D;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
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
    bf16_t* lr = rowbuf[wave];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = t * 64 * V + lane * V;
        const typename RS::fvec gv = *(const typename RS::fvec*)(gamma + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(beta + c);
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)(v[t * V + j] * rstd * gv[j] + bv[j]);
        *(typename RS::bvec*)(xr + c) = o;
        *(typename RS::bvec*)(lr + c) = o;
    }
    // the wave reads what its own lanes wrote: LDS operations of one wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // as ln_stats_canonical_rows, the row read from LDS
    constexpr int nslice = D >> 6;
    const int slice = lane >> 2, grp = lane & 3;
    float cs[2] = {0.f, 0.f}, cq[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int sl = slice + 16 * h;
        if (sl < nslice) {
            const bf16_t* sr = lr + sl * 64 + grp * 4;
            uint2 pk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pk[j] = *(const uint2*)(sr + j * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) ln_accumulate(pk[j], cs[h], cq[h]);
        }
        cs[h] += __shfl_xor(cs[h], 1, 64);
        cq[h] += __shfl_xor(cq[h], 1, 64);
        cs[h] += __shfl_xor(cs[h], 2, 64);
        cq[h] += __shfl_xor(cq[h], 2, 64);
    }
    double S = 0.0, Q = 0.0;
    for (int k = 0; k < nslice; ++k) {
        S += (double)__shfl(k < 16 ? cs[0] : cs[1], 4 * (k & 15), 64);
        Q += (double)__shfl(k < 16 ? cq[0] : cq[1], 4 * (k & 15), 64);
    }
    if (lane == 0) *(float2*)(stats + 2 * row) = ln_finish_row(S, Q, D, eps);
}

// CLIP's post_layernorm on the pooled row (modeling_clip.py, CLIPVisionTransformer.forward: pooled_output =
// self.post_layernorm(last_hidden_state[:, 0, :])): pool_ln_l2's LayerNorm of row b * 197 + tok, rounded to bf16 [B, D]
// for the projection GEMM -- no L2 step, the projected vector is what gets normalised.
template <int D>
__global__ __launch_bounds__(256) void pool_ln_rows(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int B, int tok, float eps, bf16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16_t* xr = x + ((int64_t)b * VIT_T + tok) * D;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT, NV = RS::PER_LANE;
    float v[NV];
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
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (bf16_t)(v[t * V + j] * rstd * gv[j] + bv[j]);
        *(typename RS::bvec*)(y + (int64_t)b * D + c) = o;
    }
}

// The L2 step of pool_ln_l2 on its own, for the projected rows of a CLIP tower (modeling_clip.py, CLIPModel.
// get_image_features callers normalise image_embeds: x / ||x||; here torch.nn.functional.normalize's x / max(||x||, 1e-12)
// as everywhere in this engine): f32 [rows, p] -> f32 and / or bf16.  One wave per row, p % 64 == 0, p <= 1024: a lane
// holds columns 4 lane + 256 k .. + 3.
__global__ __launch_bounds__(256) void l2_rows(const float* __restrict__ x, int64_t rows, int p, float* __restrict__ y_f32,
                                               bf16_t* __restrict__ y_bf16) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * p;
    f32x4 v[4];
    float n2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        v[k] = c < p ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
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

hipError_t launch_normalise_rows(const float* x, int64_t rows, int d, void* y, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(normalise_rows_f32, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, d, (bf16_t*)y);
    return hipGetLastError();
}

// the instantiation of a row kernel for width d (384, 768, 1024); any other width is an error, never another kernel
#define ROW_KERNEL_BY_WIDTH(d, kernel, grid, s, ...)                                                          \
    switch (d) {                                                                                              \
        case 384: hipLaunchKernelGGL(kernel<384>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 768: hipLaunchKernelGGL(kernel<768>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 1024: hipLaunchKernelGGL(kernel<1024>, grid, dim3(256), 0, s, __VA_ARGS__); break;               \
        default: return hipErrorInvalidValue;                                                                 \
    }

hipError_t launch_layernorm(const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int d, float eps, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, layernorm_rows, dim3((unsigned)((rows + 3) / 4)), s, (const bf16_t*)x, gamma, beta, (bf16_t*)y, rows, eps)
    return hipGetLastError();
}

hipError_t launch_ln_stats(const void* x, int64_t rows, int d, float eps, float* stats, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, ln_stats_rows, dim3((unsigned)((rows + 3) / 4)), s, (const bf16_t*)x, rows, eps, stats)
    return hipGetLastError();
}

hipError_t launch_ln_stats_canonical(const void* x, int64_t row0, int64_t row1, int d, float eps, float* stats, hipStream_t s, int64_t stride) {
    if (row1 <= row0) return hipSuccess;
    if (d <= 0 || (d % 64) != 0 || d > 2048 || stride < 1) return hipErrorInvalidValue;
    const int64_t nrows = (row1 - row0 + stride - 1) / stride;
    hipLaunchKernelGGL(ln_stats_canonical_rows, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, (const bf16_t*)x, row0, row1, d, eps,
                       stats, stride);
    return hipGetLastError();
}

hipError_t launch_ln_finish(const float* part, int64_t part_rows, int64_t rows, int d, float eps, float* stats, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(ln_finish_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, part, part_rows, rows, d, eps, stats);
    return hipGetLastError();
}

hipError_t launch_cls_rows(void* x, const float* cls, const float* pos, int B, int d, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, cls_rows, dim3((B + 3) / 4), s, (bf16_t*)x, cls, pos, B)
    return hipGetLastError();
}

hipError_t launch_pool(const void* x, const float* gamma, const float* beta, int B, int tok, int d, float eps, float* emb_f32,
                       void* emb_bf16, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pool_ln_l2, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tok, eps, emb_f32, (bf16_t*)emb_bf16)
    return hipGetLastError();
}

hipError_t launch_pre_ln(void* x, const float* gamma, const float* beta, int64_t rows, int d, float eps, float* stats, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pre_ln_rows, dim3((unsigned)((rows + 3) / 4)), s, (bf16_t*)x, gamma, beta, rows, eps, stats)
    return hipGetLastError();
}

hipError_t launch_pool_ln(const void* x, const float* gamma, const float* beta, int B, int tok, int d, float eps, void* y, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pool_ln_rows, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tok, eps, (bf16_t*)y)
    return hipGetLastError();
}

hipError_t launch_l2_rows(const float* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    if (p < 64 || (p % 64) != 0 || p > 1024) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(l2_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, p, y_f32, (bf16_t*)y_bf16);
    return hipGetLastError();
}
