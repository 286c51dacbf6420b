// Row-wise HBM-bound kernels of the image towers' forward and of the heads every tower ends in: LayerNorm (K3), class rows,
// the rows behind an f32 patch-embed GEMM, the pooled row's LayerNorm with and without the L2 step (K8), the L2 step alone.
//
// One 64-lane wave owns one D-wide row: 3 x 8-byte (bf16x4) loads per lane at D = 768, statistics in f32 registers, 8-byte
// stores.  Instantiated per supported width; the layout of a row over the lanes, the two-pass LayerNorm of a row and the L2
// step are row_kernels.h's.
#include "common.h"
#include "gemm_epilogue.h"
#include "kernels.h"
#include "row_kernels.h"

namespace {

template <int D>
__global__ __launch_bounds__(256) void layernorm_rows(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                      int64_t rows, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[D / 64];
    ln_row<D>(x + row * D, gamma, beta, eps, lane, v);
    row_store_bf16<D>(y + row * D, lane, v);
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
    float v[D / 64];
    row_load<D>(x + row * D, lane, v);
    const float2 st = row_stats<D>(v, eps);
    if (lane == 0) *(float2*)(stats + 2 * row) = st;
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

// The rows behind a patch-embed GEMM that ran with the f32 epilogue (acc [n * patches, D]), one rounding per value:
// x[b * TOKENS + first + p] = bf16((acc[b * patches + p] + bias) + pos[first + p]) -- the f32 order of the patch-embed
// epilogue of the 197-token path -- where first = 1 with a class token, whose row is x[b * TOKENS] = bf16(cls + pos[0]),
// and first = 0 without one (cls == nullptr); patches = TOKENS - first.
template <int N> struct Const {};  // a compile-time integer among a kernel's arguments: kernel<D> deduces it
template <int D, int TOKENS>
__global__ __launch_bounds__(256) void embed_rows(const float* __restrict__ acc, const float* __restrict__ bias, const float* __restrict__ pos,
                                                  const float* __restrict__ cls, bf16_t* __restrict__ x, int64_t rows, Const<TOKENS>) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / TOKENS;
    const int t = (int)(row - b * TOKENS);
    const int first = cls ? 1 : 0;
    const bool class_row = cls && t == 0;
    typedef RowShape<D> RS;
    constexpr int V = RS::V, NT = RS::NT;
    bf16_t* xr = x + row * D;
    const float* pr = pos + (int64_t)t * D;
    const float* ar = acc + (b * (TOKENS - first) + (class_row ? 0 : t - first)) * D;  // read for patch rows only
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int c = k * 64 * V + lane * V;
        const typename RS::fvec p = *(const typename RS::fvec*)(pr + c);
        typename RS::bvec o;
        if (class_row) {
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

// K8: restates last_pooling (deprecated_package/embedder.py:17-34) for one fixed token
// index per sequence, after the final LayerNorm of that row only (the other rows of
// the last hidden state are never read by the reference's pooling): row b * tokens + tok.
template <int D>
__global__ __launch_bounds__(256) void pool_ln_l2(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, int B, int tokens, int tok, float eps,
                                                  float* __restrict__ emb_f32, bf16_t* __restrict__ emb_bf16) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float v[D / 64];
    ln_row<D>(x + ((int64_t)b * tokens + tok) * D, gamma, beta, eps, lane, v);
    row_l2_store<D>(v, lane, emb_f32, emb_bf16, (int64_t)b * D);
}

// pool_ln_l2 over a window of token rows per crop: row (b, t), t < ntok, is the final LayerNorm and the L2 step of residual
// row b * tokens + tok0 + t -> bf16 at element (b * ntok + t) * D of y.  ln_row and row_l2_store in K8's order, so a row
// equals K8's bf16 output for pool_token = tok0 + t bit for bit.  Every offset in 64 bits (65 536 crops x 196 x 768 values).
template <int D>
__global__ __launch_bounds__(256) void token_ln_l2(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, int64_t rows, int tokens, int tok0, int ntok, float eps,
                                                   bf16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / ntok;
    const int t = (int)(row - b * ntok);
    float v[D / 64];
    ln_row<D>(x + (b * tokens + tok0 + t) * D, gamma, beta, eps, lane, v);
    row_l2_store<D>(v, lane, nullptr, y, row * D);
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
    bf16_t* lr = rowbuf[wave];
    float v[D / 64];
    ln_row<D>(xr, gamma, beta, eps, lane, v);
    row_store_bf16<D>(xr, lane, v);
    row_store_bf16<D>(lr, lane, v);
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
// self.post_layernorm(last_hidden_state[:, 0, :])): pool_ln_l2's LayerNorm of row b * tokens + tok, rounded to bf16 [B, D]
// for the projection GEMM -- no L2 step, the projected vector is what gets normalised.
template <int D>
__global__ __launch_bounds__(256) void pool_ln_rows(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int B, int tokens, int tok, float eps, bf16_t* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float v[D / 64];
    ln_row<D>(x + ((int64_t)b * tokens + tok) * D, gamma, beta, eps, lane, v);
    row_store_bf16<D>(y + (int64_t)b * D, lane, v);
}

// The L2 step of pool_ln_l2 on its own, for rows of any width p (p % 64 == 0, p <= 1024): the projected rows of a CLIP
// tower (modeling_clip.py, CLIPModel.get_image_features callers normalise image_embeds: x / ||x||; here
// torch.nn.functional.normalize's x / max(||x||, 1e-12) as everywhere in this engine), the output of SigLIP's pooling head,
// the head of a SigLIP text tower -> f32 and / or bf16 [rows, p].  One wave per row in the layout of RowShape<1024>, zeros
// at the columns >= p.  `load(i, c)`: the four f32 values of a row at column c, i = row * p + c.
struct LoadF32 {  // f32 rows
    const float* x;
    __device__ f32x4 operator()(int64_t i, int) const { return *(const f32x4*)(x + i); }
};
struct LoadBf16 {  // bf16 rows, widened
    const bf16_t* x;
    __device__ f32x4 operator()(int64_t i, int) const {
        const bf16x4 b = *(const bf16x4*)(x + i);
        return f32x4{(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
    }
};
struct LoadF32Bias {  // acc + bias[c], formed once in f32 (the rows of an EPI_F32 GEMM whose layer has a bias)
    const float* acc;
    const float* bias;
    __device__ f32x4 operator()(int64_t i, int c) const { return *(const f32x4*)(acc + i) + *(const f32x4*)(bias + c); }
};
template <class Load>
__global__ __launch_bounds__(256) void l2_rows(Load load, int64_t rows, int p, float* __restrict__ y_f32, bf16_t* __restrict__ y_bf16) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k * 256;
        const f32x4 a = c < p ? load(row * p + c, c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k * 4 + j] = a[j];
    }
    row_l2_store<1024>(v, lane, y_f32, y_bf16, row * p, p);
}

template <class Load> hipError_t launch_l2(Load load, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    if (p < 64 || (p % 64) != 0 || p > 1024) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(l2_rows<Load>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, load, rows, p, y_f32, (bf16_t*)y_bf16);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_normalise_rows(const float* x, int64_t rows, int d, void* y, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(normalise_rows_f32, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, d, (bf16_t*)y);
    return hipGetLastError();
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

static_assert(count_layouts([](const TokenLayout& L) { return L.embed_rows; }) == 3 && find_layout(50)->embed_rows && find_layout(196)->embed_rows &&
                  find_layout(257)->embed_rows, "embed_rows: instantiate the kernel for every layout whose row sets embed_rows");

hipError_t launch_embed_rows(const float* acc, const float* bias, const float* pos, const float* cls, void* x, int n, int tokens, int d, hipStream_t s) {
    const TokenLayout* L = find_layout(tokens);
    if (!vit_width_built(d) || !L || !L->embed_rows || L->cls != (cls != nullptr)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t rows = (int64_t)n * tokens;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (tokens == 50) {
        ROW_KERNEL_BY_WIDTH(d, embed_rows, grid, s, acc, bias, pos, cls, (bf16_t*)x, rows, Const<50>{})
    } else if (tokens == 196) {
        ROW_KERNEL_BY_WIDTH(d, embed_rows, grid, s, acc, bias, pos, cls, (bf16_t*)x, rows, Const<196>{})
    } else {
        ROW_KERNEL_BY_WIDTH(d, embed_rows, grid, s, acc, bias, pos, cls, (bf16_t*)x, rows, Const<257>{})
    }
    return hipGetLastError();
}

// an image layout with a pooled row, and a row of it
static bool pooled_row(int tokens, int tok) {
    const TokenLayout* L = find_layout(tokens);
    return L && L->image() && L->pooled && tok >= 0 && tok < tokens;
}

hipError_t launch_pool(const void* x, const float* gamma, const float* beta, int B, int tokens, int tok, int d, float eps, float* emb_f32,
                       void* emb_bf16, hipStream_t s) {
    if (!vit_width_built(d) || !pooled_row(tokens, tok)) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pool_ln_l2, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tokens, tok, eps, emb_f32, (bf16_t*)emb_bf16)
    return hipGetLastError();
}

hipError_t launch_token_rows(const void* x, const float* gamma, const float* beta, int n, int tokens, int tok0, int ntok, int d, float eps, void* y,
                             hipStream_t s) {
    const TokenLayout* L = find_layout(tokens);
    if (!vit_width_built(d) || !L || !L->image() || tok0 < 0 || ntok < 1 || tok0 + ntok > tokens || !y) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t rows = (int64_t)n * ntok;
    ROW_KERNEL_BY_WIDTH(d, token_ln_l2, dim3((unsigned)((rows + 3) / 4)), s, (const bf16_t*)x, gamma, beta, rows, tokens, tok0, ntok, eps, (bf16_t*)y)
    return hipGetLastError();
}

hipError_t launch_pre_ln(void* x, const float* gamma, const float* beta, int64_t rows, int d, float eps, float* stats, hipStream_t s) {
    if (!vit_width_built(d)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pre_ln_rows, dim3((unsigned)((rows + 3) / 4)), s, (bf16_t*)x, gamma, beta, rows, eps, stats)
    return hipGetLastError();
}

hipError_t launch_pool_ln(const void* x, const float* gamma, const float* beta, int B, int tokens, int tok, int d, float eps, void* y, hipStream_t s) {
    if (!vit_width_built(d) || !pooled_row(tokens, tok)) return hipErrorInvalidValue;
    if (B <= 0) return hipSuccess;
    ROW_KERNEL_BY_WIDTH(d, pool_ln_rows, dim3((B + 3) / 4), s, (const bf16_t*)x, gamma, beta, B, tokens, tok, eps, (bf16_t*)y)
    return hipGetLastError();
}

hipError_t launch_l2_rows(const float* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    return launch_l2(LoadF32{x}, rows, p, y_f32, y_bf16, s);
}
hipError_t launch_l2_rows_bf16(const void* x, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    return launch_l2(LoadBf16{(const bf16_t*)x}, rows, p, y_f32, y_bf16, s);
}
hipError_t launch_bias_l2_rows(const float* acc, const float* bias, int64_t rows, int p, float* y_f32, void* y_bf16, hipStream_t s) {
    return launch_l2(LoadF32Bias{acc, bias}, rows, p, y_f32, y_bf16, s);
}
