// Kernels of the Mllama language tower (capi_mllama.hip): transformers models/mllama/modeling_mllama.py,
// MllamaTextModel with its self-attention and cross-attention decoder layers, heads of 128.
//   row kernels   token gather, RMSNorm of a row, RMSNorm of every 128-wide head (q_norm / k_norm), RoPE in the rotate_half
//                 form on the Q | K heads, silu(gate) * up, and the final norm + pooling + L2 of row len - 1.  All statistics
//                 are f32 over the bf16 inputs, every output value is rounded once.
//   mllama_self_attn    causal GQA attention, S <= 128: a wave per query row, a lane per key for the scores (f32 dot over
//                 the 128 values), a lane per pair of output columns for P . V.  P stays f32.
//   mllama_cross_attn_partial / _merge   the hot kernel: per (image, KV head) the group * S query rows against the T * P
//                 projected vision rows.  S^T = K . Q^T and O^T = V^T . P^T on mfma_f32_16x16x32_bf16, online softmax in
//                 f32 (base 2), the per-row tile mask applied to the scores by SELECTION.  The key axis is cut into splits
//                 of CROSS_SPLIT_TILES tiles of 32 keys -- a function of the key count alone --, one workgroup per split,
//                 which leaves (max, sum, O) per query row; the merge launch combines the splits in ascending order, so
//                 that the result does not depend on the chunk or on the launch.
//                 P is rounded to bf16 for P . V, the sum runs over the f32 P (as attention.hip), the output is rounded once.
#include "common.h"
#include "kernels.h"
#include "mllama_lm.h"

namespace {

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// x[r, :] = tok[ids[r], :]
__global__ __launch_bounds__(256) void mllama_gather(const bf16_t* __restrict__ tok, const int32_t* __restrict__ ids, bf16_t* __restrict__ x, const int d) {
    const size_t r = blockIdx.x;
    const uint4* src = (const uint4*)(tok + (size_t)ids[r] * d);
    uint4* dst = (uint4*)(x + r * d);
    for (int i = threadIdx.x; i < d / 8; i += 256) dst[i] = src[i];
}

// y[r, :] = bf16(w * (x[r, :] * rsqrt(mean(x^2) + eps)))
__global__ __launch_bounds__(256) void mllama_rmsnorm(const bf16_t* __restrict__ x, const float* __restrict__ w, bf16_t* __restrict__ y, const int d,
                                                      const float eps) {
    __shared__ float red[4];
    const size_t r = blockIdx.x;
    const bf16x8* xr = (const bf16x8*)(x + r * d);
    float ss = 0.f;
    for (int i = threadIdx.x; i < d / 8; i += 256) {
        const bf16x8 v = xr[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (float)v[e] * (float)v[e];
    }
    const float rstd = rsqrtf(block_sum_256(ss, red) / (float)d + eps);
    bf16x8* yr = (bf16x8*)(y + r * d);
    for (int i = threadIdx.x; i < d / 8; i += 256) {
        const bf16x8 v = xr[i];
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16_t)(w[i * 8 + e] * ((float)v[e] * rstd));
        yr[i] = o;
    }
}

// in place: every head of 128 of row r (heads of them from column col0 on, rows of ld values) is RMS-normalised with w [128]
__global__ __launch_bounds__(256) void mllama_headnorm(bf16_t* __restrict__ x, const float* __restrict__ w, const int64_t items, const int heads,
                                                       const int64_t ld, const int col0, const float eps) {
    const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= items) return;
    const int lane = threadIdx.x & 63;
    const int64_t r = it / heads;
    const int h = (int)(it - r * heads);
    bf16x2* p = (bf16x2*)(x + r * ld + col0 + h * 128) + lane;
    const bf16x2 v = *p;
    const float a = (float)v[0], b = (float)v[1];
    const float rstd = rsqrtf(wave_sum(a * a + b * b) * (1.0f / 128.0f) + eps);
    bf16x2 o;
    o[0] = (bf16_t)(w[2 * lane] * (a * rstd));
    o[1] = (bf16_t)(w[2 * lane + 1] * (b * rstd));
    *p = o;
}

// in place on the first `heads` heads of every row (Q | K): rotate_half RoPE at position r % S; cs / sn f32 [128, 64]
__global__ __launch_bounds__(256) void mllama_rope(bf16_t* __restrict__ x, const float* __restrict__ cs, const float* __restrict__ sn, const int64_t items,
                                                   const int heads, const int64_t ld, const int S) {
    const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= items) return;
    const int lane = threadIdx.x & 63;
    const int64_t r = it / heads;
    const int h = (int)(it - r * heads);
    const int pos = (int)(r % S);
    bf16_t* p = x + r * ld + h * 128;
    const float a = (float)p[lane], b = (float)p[lane + 64];
    const float c = cs[pos * 64 + lane], s = sn[pos * 64 + lane];
    p[lane] = (bf16_t)(a * c - b * s);
    p[lane + 64] = (bf16_t)(b * c + a * s);
}

// act[r, i] = bf16(silu(gu[r, i]) * gu[r, I + i]); a row with rowzero[r] != 0 is written as zeros
__global__ __launch_bounds__(256) void mllama_silu_mul(const bf16_t* __restrict__ gu, bf16_t* __restrict__ act, const uint8_t* __restrict__ rowzero,
                                                       const int I) {
    const size_t r = blockIdx.x;
    const bool zero = rowzero && rowzero[r];
    const bf16x8* g = (const bf16x8*)(gu + r * 2 * I);
    const bf16x8* u = (const bf16x8*)(gu + r * 2 * I + I);
    bf16x8* o = (bf16x8*)(act + r * I);
    for (int i = threadIdx.x; i < I / 8; i += 256) {
        const bf16x8 a = g[i], b = u[i];
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ga = (float)a[e];
            v[e] = zero ? (bf16_t)0.f : (bf16_t)((ga / (1.0f + __expf(-ga))) * (float)b[e]);
        }
        o[i] = v;
    }
}

// row b * S + len[b] - 1: v = w * (x * rstd) in f32, then v / max(||v||, 1e-12)
__global__ __launch_bounds__(256) void mllama_pool(const bf16_t* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ len, const int S,
                                                   const int d, const float eps, float* __restrict__ ef, bf16_t* __restrict__ eb) {
    __shared__ float red[4];
    const size_t b = blockIdx.x;
    const bf16_t* xr = x + (b * S + (len[b] - 1)) * d;
    float ss = 0.f;
    for (int i = threadIdx.x; i < d; i += 256) ss += (float)xr[i] * (float)xr[i];
    const float rstd = rsqrtf(block_sum_256(ss, red) / (float)d + eps);
    float nn = 0.f;
    for (int i = threadIdx.x; i < d; i += 256) {
        const float v = w[i] * ((float)xr[i] * rstd);
        nn += v * v;
    }
    const float inv = 1.0f / fmaxf(sqrtf(block_sum_256(nn, red)), 1e-12f);
    for (int i = threadIdx.x; i < d; i += 256) {
        const float v = w[i] * ((float)xr[i] * rstd) * inv;
        if (ef) ef[b * d + i] = v;
        if (eb) eb[b * d + i] = (bf16_t)v;
    }
}

// the tile tower's final state and its ni intermediate states (rows padded to 1608 per tile) -> bf16 [rows, 1280 (1 + ni)] in
// the feature order of launch_tile_output: [0, 1280) the final state, 1280 + d ni + k state k's value d
__global__ __launch_bounds__(256) void mllama_tile_states(const bf16_t* __restrict__ x, const bf16_t* __restrict__ inter, const int ni,
                                                          const int64_t inter_stride, bf16_t* __restrict__ out) {
    const int64_t r = blockIdx.x;
    const int64_t src = r / 1601 * 1608 + r % 1601;
    const int F = 1280 * (1 + ni);
    bf16_t* o = out + r * F;
    for (int f = threadIdx.x; f < F; f += 256) {
        if (f < 1280) o[f] = x[src * 1280 + f];
        else {
            const int j = f - 1280, d = j / ni, k = j - d * ni;
            o[f] = inter[k * inter_stride + src * 1280 + d];
        }
    }
}

// qkv [n S, (H + 2 KVH) 128] (Q | K | V, RoPE applied) -> out [n S, H 128]; a wave per (sequence, head, row); rows >= len are zero
__global__ __launch_bounds__(256) void mllama_self_attn(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int32_t* __restrict__ len,
                                                        const int64_t items, const int S, const int H, const int KVH, const float scale2) {
    const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= items) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(it % S);
    const int64_t bh = it / S;
    const int h = (int)(bh % H);
    const int64_t b = bh / H;
    const int64_t ld = (int64_t)(H + 2 * KVH) * 128;
    const int kvh = h / (H / KVH);
    bf16_t* o = out + ((b * S + i) * H + h) * 128;
    if (i >= len[b]) {
        o[lane] = (bf16_t)0.f;
        o[lane + 64] = (bf16_t)0.f;
        return;
    }
    const bf16_t* kbase = qkv + b * S * ld + (int64_t)(H + kvh) * 128;
    const bf16_t* vbase = kbase + (int64_t)KVH * 128;
    const bf16x8* q = (const bf16x8*)(qkv + (b * S + i) * ld + (int64_t)h * 128);
    float sc[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = lane + 64 * half;
        float a = 0.f;
        if (j <= i) {
            const bf16x8* k = (const bf16x8*)(kbase + j * ld);
#pragma unroll 4
            for (int c = 0; c < 16; ++c) {
                const bf16x8 kv = k[c], qv = q[c];
#pragma unroll
                for (int e = 0; e < 8; ++e) a += (float)qv[e] * (float)kv[e];
            }
        }
        sc[half] = j <= i ? a * scale2 : -INFINITY;
    }
    const float mx = wave_max(fmaxf(sc[0], sc[1]));  // key 0 counts for every row: mx is a score
    const float p0 = __builtin_amdgcn_exp2f(sc[0] - mx), p1 = __builtin_amdgcn_exp2f(sc[1] - mx);  // exp2(-inf) = 0
    const float inv = 1.0f / wave_sum(p0 + p1);
    float o0 = 0.f, o1 = 0.f;
    for (int j = 0; j <= i; ++j) {
        const float p = __shfl(j < 64 ? p0 : p1, j & 63, 64);
        o0 += p * (float)vbase[j * ld + lane];
        o1 += p * (float)vbase[j * ld + lane + 64];
    }
    o[lane] = (bf16_t)(o0 * inv);
    o[lane + 64] = (bf16_t)(o1 * inv);
}

constexpr int KROW = 272;  // bytes of a key row in LDS: 256 + 16, so that the 16 rows of a fragment read fall in different banks
constexpr int VROW = 80;   // bytes of a row of V^T in LDS: 32 keys + 16

// One split of the key axis for one (image, KV head): partial (max, sum, O) of every query row r = g * S + s (head kvh * G + g,
// position s).  part_m / part_l [slot, R], part_o [slot, R, 128], slot = (img * KVH + kvh) * nsplit + split.  The maximum is
// in base-2 units (scale2 = dh^-0.5 log2 e).  xm [n S]: the tiles a row attends as bits; 0 = every tile (the fully masked
// row of transformers' _prepare_cross_attention_mask, whose additive mask is multiplied to zero).
__global__ __launch_bounds__(256) void mllama_cross_attn_partial(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv, const uint8_t* __restrict__ xm,
                                                                 float* __restrict__ part_m, float* __restrict__ part_l, float* __restrict__ part_o,
                                                                 const int S, const int G, const int KVH, const int Nk, const int P, const int T,
                                                                 const int nsplit, const float scale2) {
    __shared__ __attribute__((aligned(16))) char Kl[32 * KROW];
    __shared__ __attribute__((aligned(16))) char Vl[128 * VROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x, kvh = blockIdx.y, img = blockIdx.z;
    const int H = G * KVH, R = G * S, nqb = (R + 15) >> 4;
    const int ntiles = (Nk + 31) >> 5;
    const int t0 = split * CROSS_SPLIT_TILES, t1 = min(t0 + CROSS_SPLIT_TILES, ntiles);
    const int64_t ldkv = (int64_t)2 * KVH * 128;
    const bf16_t* kimg = kv + (int64_t)img * Nk * ldkv + kvh * 128;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t slot = ((int64_t)img * KVH + kvh) * nsplit + split;
    for (int qg = 0; qg < nqb; qg += 4) {
        const int qb = qg + wave;
        const bool active = qb < nqb;  // wave-uniform
        const int r_raw = qb * 16 + l15;
        const int r = min(r_raw, R - 1);
        const int g = r / S, s = r - g * S;
        const bf16_t* qp = q + (((int64_t)img * S + s) * H + kvh * G + g) * 128 + 8 * l4;
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + 32 * ks);
        int bits = xm[(int64_t)img * S + s];
        if (bits == 0) bits = (1 << T) - 1;
        float m = -INFINITY, l = 0.f;
        f32x4 o[8];
#pragma unroll
        for (int db = 0; db < 8; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = t0; kt < t1; ++kt) {
            __syncthreads();  // every wave is done with the previous tile
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int idx = tid + 256 * c;  // 32 keys x 16 pieces of 8 values
                const int key = idx >> 4, piece = idx & 15;
                const int kg = min(kt * 32 + key, Nk - 1);  // a key past the end is a clamped copy; its P is 0 by selection
                const bf16_t* src = kimg + kg * ldkv + piece * 8;
                *(uint4*)(Kl + key * KROW + piece * 16) = *(const uint4*)src;
                const bf16x8 vv = *(const bf16x8*)(src + KVH * 128);
                const int kidx = 8 * ((key >> 2) & 3) + 4 * (key >> 4) + (key & 3);  // the order of P's values in a lane (below)
#pragma unroll
                for (int e = 0; e < 8; ++e) *(bf16_t*)(Vl + (piece * 8 + e) * VROW + kidx * 2) = vv[e];
            }
            __syncthreads();
            if (!active) continue;
            float v[8];
            bool ok[8];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *(const bf16x8*)(Kl + (16 * t + l15) * KROW + (32 * ks + 8 * l4) * 2);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // S^T[key 16 t + 4 l4 + i][query l15]
                    const int key = kt * 32 + 16 * t + 4 * l4 + i;
                    ok[4 * t + i] = key < Nk && ((bits >> (key / P)) & 1);
                    v[4 * t + i] = ok[4 * t + i] ? acc[i] * scale2 : -INFINITY;
                }
            }
            float tm = v[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) tm = fmaxf(tm, v[j]);
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m, tm);
            const bool none = mn == -INFINITY;  // no key of this row has counted so far
            const float alpha = none ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
            bf16x8 pf;
            float ps = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = (ok[j] && !none) ? __builtin_amdgcn_exp2f(v[j] - mn) : 0.f;
                ps += p;
                pf[j] = (bf16_t)p;
            }
            ps += __shfl_xor(ps, 16, 64);
            ps += __shfl_xor(ps, 32, 64);
            l = l * alpha + ps;
            m = mn;
#pragma unroll
            for (int db = 0; db < 8; ++db) {  // O^T[value 16 db + 4 l4 + i][query l15]
                const bf16x8 vf = *(const bf16x8*)(Vl + (16 * db + l15) * VROW + 16 * l4);
                f32x4 a = o[db];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] *= alpha;
                o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, a, 0, 0, 0);
            }
        }
        if (active && r_raw < R) {
            const int64_t row = slot * R + r_raw;
            if (l4 == 0) {
                part_m[row] = m;
                part_l[row] = l;
            }
#pragma unroll
            for (int db = 0; db < 8; ++db) *(f32x4*)(part_o + row * 128 + 16 * db + 4 * l4) = o[db];
        }
    }
}

// the splits of one query row, in ascending order -> out [n S, H 128]; a wave per (image, KV head, row)
__global__ __launch_bounds__(64) void mllama_cross_attn_merge(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                              const float* __restrict__ part_o, bf16_t* __restrict__ out, const int S, const int G,
                                                              const int KVH, const int nsplit) {
    const int R = G * S, lane = threadIdx.x;
    const int r = blockIdx.x, kvh = blockIdx.y, img = blockIdx.z;
    const int64_t slot0 = ((int64_t)img * KVH + kvh) * nsplit;
    float M = -INFINITY;
    for (int z = 0; z < nsplit; ++z) M = fmaxf(M, part_m[(slot0 + z) * R + r]);
    float L = 0.f, o0 = 0.f, o1 = 0.f;
    for (int z = 0; z < nsplit; ++z) {
        const int64_t row = (slot0 + z) * R + r;
        const float mz = part_m[row];
        if (mz == -INFINITY) continue;  // no key of this split counted for the row
        const float w = __builtin_amdgcn_exp2f(mz - M);
        L += part_l[row] * w;
        o0 += part_o[row * 128 + lane] * w;
        o1 += part_o[row * 128 + lane + 64] * w;
    }
    const float inv = 1.0f / L;
    const int g = r / S, s = r - g * S;
    bf16_t* o = out + (((int64_t)img * S + s) * (G * KVH) + kvh * G + g) * 128;
    o[lane] = (bf16_t)(o0 * inv);
    o[lane + 64] = (bf16_t)(o1 * inv);
}

}  // namespace

hipError_t launch_mllama_gather(const void* tok, const int32_t* ids, void* x, int64_t rows, int d, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (d % 8 || rows > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_gather, dim3((unsigned)rows), dim3(256), 0, s, (const bf16_t*)tok, ids, (bf16_t*)x, d);
    return hipGetLastError();
}

hipError_t launch_mllama_rmsnorm(const void* x, const float* w, void* y, int64_t rows, int d, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (d % 8 || rows > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_rmsnorm, dim3((unsigned)rows), dim3(256), 0, s, (const bf16_t*)x, w, (bf16_t*)y, d, eps);
    return hipGetLastError();
}

hipError_t launch_mllama_headnorm(void* x, const float* w, int64_t rows, int heads, int64_t ld, int col0, float eps, hipStream_t s) {
    const int64_t items = rows * heads;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > 0x7fffffff || ld % 2 || col0 % 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_headnorm, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (bf16_t*)x, w, items, heads, ld, col0, eps);
    return hipGetLastError();
}

hipError_t launch_mllama_rope(void* x, const float* cs, const float* sn, int64_t rows, int heads, int64_t ld, int S, hipStream_t s) {
    const int64_t items = rows * heads;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > 0x7fffffff || S < 1 || S > MLLAMA_MAX_S) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_rope, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (bf16_t*)x, cs, sn, items, heads, ld, S);
    return hipGetLastError();
}

hipError_t launch_mllama_silu_mul(const void* gu, void* act, const uint8_t* rowzero, int64_t rows, int I, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (I % 8 || rows > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_silu_mul, dim3((unsigned)rows), dim3(256), 0, s, (const bf16_t*)gu, (bf16_t*)act, rowzero, I);
    return hipGetLastError();
}

hipError_t launch_mllama_pool(const void* x, const float* w, const int32_t* len, int n, int S, int d, float eps, float* ef, void* eb, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mllama_pool, dim3((unsigned)n), dim3(256), 0, s, (const bf16_t*)x, w, len, S, d, eps, ef, (bf16_t*)eb);
    return hipGetLastError();
}

hipError_t launch_mllama_tile_states(const void* x, const void* inter, int ni, int64_t inter_stride, void* out, int64_t rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (rows > 0x7fffffff || ni < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mllama_tile_states, dim3((unsigned)rows), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)inter, ni, inter_stride, (bf16_t*)out);
    return hipGetLastError();
}

hipError_t launch_mllama_self_attn(const void* qkv, void* out, const int32_t* len, int n, int S, int H, int KVH, hipStream_t s) {
    const int64_t items = (int64_t)n * H * S;
    if (items <= 0) return hipSuccess;
    if (S > MLLAMA_MAX_S || KVH < 1 || H % KVH || (items + 3) / 4 > 0x7fffffff) return hipErrorInvalidValue;
    const float scale2 = 0.08838834764831845f * 1.44269504088896341f;  // 128^-0.5 log2 e
    hipLaunchKernelGGL(mllama_self_attn, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, (const bf16_t*)qkv, (bf16_t*)out, len, items, S, H, KVH, scale2);
    return hipGetLastError();
}

int mllama_cross_splits(int Nk) { return ((Nk + 31) / 32 + CROSS_SPLIT_TILES - 1) / CROSS_SPLIT_TILES; }

size_t mllama_cross_workspace_floats(int n, int S, int H, int Nk) { return (size_t)n * H * S * mllama_cross_splits(Nk) * 130 + 8; }

hipError_t launch_mllama_cross_attn(const void* q, const void* kv, const uint8_t* xm, void* out, float* ws, int n, int S, int H, int KVH, int T, int P,
                                    hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (S < 1 || S > MLLAMA_MAX_S || KVH < 1 || H % KVH || T < 1 || T > 4 || P < 1 || KVH > 65535 || n > 65535) return hipErrorInvalidValue;
    const int G = H / KVH, Nk = T * P, nsplit = mllama_cross_splits(Nk);
    const size_t rows = (size_t)n * H * S * nsplit;  // (slot, r) pairs
    const size_t rows4 = (rows + 3) & ~(size_t)3;  // part_o stays 16-byte aligned
    float *pm = ws, *pl = ws + rows4, *po = ws + 2 * rows4;
    const float scale2 = 0.08838834764831845f * 1.44269504088896341f;
    hipLaunchKernelGGL(mllama_cross_attn_partial, dim3(nsplit, KVH, n), dim3(256), 0, s, (const bf16_t*)q, (const bf16_t*)kv, xm, pm, pl, po, S, G, KVH, Nk, P,
                       T, nsplit, scale2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mllama_cross_attn_merge, dim3(G * S, KVH, n), dim3(64), 0, s, pm, pl, po, (bf16_t*)out, S, G, KVH, nsplit);
    return hipGetLastError();
}
