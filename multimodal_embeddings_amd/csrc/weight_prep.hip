// Device-side weight preparation: the kernels behind DevPrep (ctx.h, weight_load.hip), over a staged copy of the
// checkpoint's own bytes (f32, bf16 or f16).  Every kernel keeps the operations of HostPrep's loop for the same buffer and
// their order, so the prepared buffers are bit-identical to the host preparer's (tests/test_gpu_checkpoint.py compares
// their fingerprints):
//   convert  dtype -> f32 (exact), optional f32 scale, -> f32 table or -> bf16 (round to nearest even); a NaN leaves quiet;
//            the parts of a concatenated buffer (Q | K | V) are one launch each into their slice of it
//   pad      [rows, cols] -> bf16 [rows, cols_padded], zero columns behind
//   rowscale [rows, cols] times a per-row factor (LayerScale folded into the projection it follows): f32(factor[row] * w), then
//            -> bf16 (round to nearest even); mul is the same product element by element as an f32 table (the bias)
//   fold     LayerNorm folding: W' = bf16(w * gamma), colsum = sum_k W', bias' = b + sum_k w * beta; the two sums run over k
//            ASCENDING in one f64 accumulator per output row (a row per thread; a tree reduction would change the order)
//   fingerprint  position-dependent 64-bit checksum of a buffer's bytes (integer adds: the reduction order is free)
// No fast-math and no flushing of f32 subnormals in this file: the results must match IEEE host arithmetic.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.h"

namespace {

constexpr int WP_THREADS = 256;
constexpr int WP_MAX_BLOCKS = 2048;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// f32_to_bf16_rne of ctx.h, bit for bit
__device__ __forceinline__ uint32_t bf16_rne_bits(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

__device__ __forceinline__ uint32_t quiet_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u ? (u | 0x00400000u) : u; }

// eight consecutive elements of `dt` from a 16-byte aligned address -> f32 (exact for all three types)
template <int DT>
__device__ __forceinline__ void load8(const void* base, size_t elem, float v[8]) {
    if (DT == MME_DT_F32) {
        const f32x4* p = (const f32x4*)((const float*)base + elem);
        const f32x4 a = p[0], b = p[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = a[j];
            v[4 + j] = b[j];
        }
    } else {
        const u32x4 r = *(const u32x4*)((const uint16_t*)base + elem);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t lo = r[j] & 0xffffu, hi = r[j] >> 16;
            if (DT == MME_DT_BF16) {
                v[2 * j] = __uint_as_float(lo << 16);
                v[2 * j + 1] = __uint_as_float(hi << 16);
            } else {
                const uint16_t l16 = (uint16_t)lo, h16 = (uint16_t)hi;
                _Float16 hl, hh;
                __builtin_memcpy(&hl, &l16, 2);
                __builtin_memcpy(&hh, &h16, 2);
                v[2 * j] = (float)hl;
                v[2 * j + 1] = (float)hh;
            }
        }
    }
}

__device__ __forceinline__ u32x4 pack8_bf16(const float v[8]) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bf16_rne_bits(v[2 * j]) | (bf16_rne_bits(v[2 * j + 1]) << 16);
    return o;
}

struct ConvertArgs {
    const void* src;
    unsigned long long chunks;  // of 8 elements
    float scale;
    int scaled;    // multiply by `scale` (the load sequences say where; HostPrep skips the multiplication elsewhere too)
    int out_bf16;  // else an f32 table
    void* dst;
};

template <int DT>
__global__ __launch_bounds__(WP_THREADS) void convert_kernel(ConvertArgs a) {
    for (unsigned long long c = (unsigned long long)blockIdx.x * WP_THREADS + threadIdx.x; c < a.chunks; c += (unsigned long long)gridDim.x * WP_THREADS) {
        float v[8];
        load8<DT>(a.src, (size_t)c * 8, v);
        if (a.scaled) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * a.scale;
        }
        if (a.out_bf16) {
            ((u32x4*)a.dst)[c] = pack8_bf16(v);
        } else {
            // a NaN leaves as a quiet NaN on this path too (an unscaled f32 or bf16 value is moved by integer operations
            // only, which would hand a signalling NaN through; f32_quiet_nan of ctx.h is the host form)
            u32x4 lo, hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo[j] = quiet_nan_bits(__float_as_uint(v[j]));
                hi[j] = quiet_nan_bits(__float_as_uint(v[4 + j]));
            }
            ((u32x4*)a.dst)[2 * c] = lo;
            ((u32x4*)a.dst)[2 * c + 1] = hi;
        }
    }
}

// [rows, cols] -> bf16 [rows, colsp]; four elements per thread (cols % 4 == 0, colsp % 4 == 0: a row of 588 16-bit
// elements starts 8-byte aligned only)
template <int DT>
__global__ __launch_bounds__(WP_THREADS) void pad_kernel(const void* src, int rows, int cols, int colsp, uint16_t* dst) {
    const int q = colsp / 4;
    const long long total = (long long)rows * q;
    for (long long i = (long long)blockIdx.x * WP_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * WP_THREADS) {
        const int r = (int)(i / q), k = (int)(i % q) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (k < cols) {
            const size_t e = (size_t)r * cols + k;
            if (DT == MME_DT_F32) {
                const f32x4 a = *(const f32x4*)((const float*)src + e);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = a[j];
            } else {
                const uint2 w = *(const uint2*)((const uint16_t*)src + e);
                const uint32_t h[4] = {w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (DT == MME_DT_BF16) {
                        v[j] = __uint_as_float(h[j] << 16);
                    } else {
                        const uint16_t b = (uint16_t)h[j];
                        _Float16 x;
                        __builtin_memcpy(&x, &b, 2);
                        v[j] = (float)x;
                    }
                }
            }
        }
        uint2 o;
        o.x = bf16_rne_bits(v[0]) | (bf16_rne_bits(v[1]) << 16);
        o.y = bf16_rne_bits(v[2]) | (bf16_rne_bits(v[3]) << 16);
        *(uint2*)(dst + (size_t)r * colsp + k) = o;
    }
}

// one element of `dt` -> f32 (exact)
template <int DT>
__device__ __forceinline__ float load1(const void* base, size_t elem) {
    if (DT == MME_DT_F32) return ((const float*)base)[elem];
    if (DT == MME_DT_BF16) return __uint_as_float((uint32_t)((const uint16_t*)base)[elem] << 16);
    return (float)((const _Float16*)base)[elem];
}

// chunks of 8 elements of a [rows, cols] matrix (cols % 8 == 0: a chunk lies in one row), each times its row's factor
template <int DT>
__global__ __launch_bounds__(WP_THREADS) void rowscale_kernel(const void* src, unsigned long long chunks, unsigned long long cols, const void* factor,
                                                              void* dst) {
    for (unsigned long long c = (unsigned long long)blockIdx.x * WP_THREADS + threadIdx.x; c < chunks; c += (unsigned long long)gridDim.x * WP_THREADS) {
        float v[8];
        load8<DT>(src, (size_t)c * 8, v);
        const float f = load1<DT>(factor, (size_t)(c * 8 / cols));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f * v[j];  // rounded to f32 here (as HostPrep::rowscaled)
        ((u32x4*)dst)[c] = pack8_bf16(v);
    }
}

template <int DT>
__global__ __launch_bounds__(WP_THREADS) void mul_kernel(const void* src, const void* factor, unsigned long long n, float* dst) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * WP_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * WP_THREADS)
        dst[i] = __uint_as_float(quiet_nan_bits(__float_as_uint(load1<DT>(factor, i) * load1<DT>(src, i))));
}

// ---- fold --------------------------------------------------------------------------------------------------------------
// One wave per 64 output rows, a row per thread.  The [64 rows x 64 k] tile comes through LDS: coalesced 16-byte global
// loads (a row's 64 k are 128 / 256 contiguous bytes), converted and scaled on the way in, then every thread walks ITS row
// k ascending with 16-byte LDS reads (rows padded by one access width).  The rounded W' goes back through LDS the same way
// so that the global stores are 16 bytes wide as well.
constexpr int FOLD_ROWS = 64, FOLD_KT = 64, FOLD_MAXK = 1280;
constexpr int FOLD_WLD = FOLD_KT + 4;  // f32 row pitch: 272 bytes
constexpr int FOLD_QLD = FOLD_KT + 8;  // bf16 row pitch: 144 bytes

struct FoldArgs {
    WpFoldSrc src[3];
    int rows_end[3];  // running total of rows
    int nsrc, cols;
    const void *gamma, *beta;
    uint16_t* wf;
    float *cs, *bf;
};

template <int DT>
__global__ __launch_bounds__(FOLD_ROWS) void fold_kernel(FoldArgs a) {
    __shared__ __attribute__((aligned(16))) float w_s[FOLD_ROWS * FOLD_WLD];
    __shared__ __attribute__((aligned(16))) uint16_t q_s[FOLD_ROWS * FOLD_QLD];
    __shared__ __attribute__((aligned(16))) float g_s[FOLD_MAXK];
    __shared__ __attribute__((aligned(16))) float b_s[FOLD_MAXK];
    const int tid = threadIdx.x, row0 = blockIdx.x * FOLD_ROWS, K = a.cols;
    int i = 0, first = 0;
    if (a.nsrc > 1 && row0 >= a.rows_end[0]) { i = 1; first = a.rows_end[0]; }
    if (a.nsrc > 2 && row0 >= a.rows_end[1]) { i = 2; first = a.rows_end[1]; }
    const WpFoldSrc S = a.src[i];
    const int lrow0 = row0 - first;  // the block's first row inside its source (sources hold whole blocks of rows)
    for (int c = tid; c < K / 8; c += FOLD_ROWS) {
        float v[8];
        load8<DT>(a.gamma, (size_t)c * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) g_s[c * 8 + j] = v[j];
        load8<DT>(a.beta, (size_t)c * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) b_s[c * 8 + j] = v[j];
    }
    double s = 0.0, t = 0.0;
    for (int k0 = 0; k0 < K; k0 += FOLD_KT) {
        __syncthreads();  // the previous tile has been read (and g_s / b_s are there)
#pragma unroll
        for (int it = 0; it < FOLD_ROWS * FOLD_KT / 8 / FOLD_ROWS; ++it) {
            const int c = it * FOLD_ROWS + tid, r = c >> 3, k8 = (c & 7) * 8;
            float v[8];
            load8<DT>(S.w, (size_t)(lrow0 + r) * K + k0 + k8, v);
            if (S.scaled) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = v[j] * S.scale;  // rounded to f32 HERE, before gamma (as HostPrep::folded)
            }
            f32x4 lo, hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo[j] = v[j];
                hi[j] = v[4 + j];
            }
            *(f32x4*)&w_s[r * FOLD_WLD + k8] = lo;
            *(f32x4*)&w_s[r * FOLD_WLD + k8 + 4] = hi;
        }
        __syncthreads();
#pragma unroll 2
        for (int k8 = 0; k8 < FOLD_KT; k8 += 8) {
            const f32x4 lo = *(const f32x4*)&w_s[tid * FOLD_WLD + k8], hi = *(const f32x4*)&w_s[tid * FOLD_WLD + k8 + 4];
            float q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float w = j < 4 ? lo[j] : hi[j - 4];
                const uint32_t qb = bf16_rne_bits(w * g_s[k0 + k8 + j]);
                q[j] = __uint_as_float(qb << 16);
                s += (double)q[j];
                t += (double)w * (double)b_s[k0 + k8 + j];
            }
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (__float_as_uint(q[2 * j]) >> 16) | (__float_as_uint(q[2 * j + 1]) & 0xffff0000u);
            *(u32x4*)&q_s[tid * FOLD_QLD + k8] = o;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < FOLD_ROWS * FOLD_KT / 8 / FOLD_ROWS; ++it) {
            const int c = it * FOLD_ROWS + tid, r = c >> 3, k8 = (c & 7) * 8;
            *(u32x4*)(a.wf + (size_t)(row0 + r) * K + k0 + k8) = *(const u32x4*)&q_s[r * FOLD_QLD + k8];
        }
    }
    double b = 0.0;
    if (S.b) {
        float bv;
        const size_t e = (size_t)lrow0 + tid;
        if (DT == MME_DT_F32) {
            bv = ((const float*)S.b)[e];
        } else if (DT == MME_DT_BF16) {
            bv = __uint_as_float((uint32_t)((const uint16_t*)S.b)[e] << 16);
        } else {
            bv = (float)((const _Float16*)S.b)[e];
        }
        if (S.scaled) bv = bv * S.scale;
        b = (double)bv;
    }
    a.cs[row0 + tid] = (float)s;
    a.bf[row0 + tid] = (float)(b + t);
}

// ---- fingerprint ---------------------------------------------------------------------------------------------------------
struct FpBuf {
    const void* p;
    unsigned long long bytes;
};

__device__ __forceinline__ unsigned long long odd_hash(unsigned long long x) {  // splitmix64 finaliser, forced odd
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (x ^ (x >> 31)) | 1ull;
}

constexpr int FP_BLOCKS = 64;

// grid (FP_BLOCKS, buffers): out[b] += sum over the buffer's 32-bit words of word * odd_hash(word index), mod 2^64
__global__ __launch_bounds__(WP_THREADS) void fingerprint_kernel(const FpBuf* bufs, unsigned long long* out) {
    __shared__ unsigned long long part[WP_THREADS / 64];
    const FpBuf B = bufs[blockIdx.y];
    const unsigned long long words = B.bytes / 4, vecs = words / 4;
    unsigned long long acc = 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * WP_THREADS + threadIdx.x; v < vecs; v += (unsigned long long)FP_BLOCKS * WP_THREADS) {
        const u32x4 w = ((const u32x4*)B.p)[v];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (unsigned long long)w[j] * odd_hash(4 * v + j);
    }
    if (blockIdx.x == 0) {
        const unsigned long long wi = vecs * 4 + threadIdx.x;  // at most three whole words behind the last 16 bytes
        if (threadIdx.x < 4 && wi < words) acc += (unsigned long long)((const uint32_t*)B.p)[wi] * odd_hash(wi);
        if (threadIdx.x == 4 && (B.bytes & 3)) {  // and at most three bytes behind the last word
            uint32_t w = 0;
            for (unsigned k = 0; k < (B.bytes & 3); ++k) w |= (uint32_t)((const uint8_t*)B.p)[words * 4 + k] << (8 * k);
            acc += (unsigned long long)w * odd_hash(words);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int k = 0; k < WP_THREADS / 64; ++k) sum += part[k];
        if (sum) atomicAdd(out + blockIdx.y, sum);
    }
}

int grid_for(unsigned long long items) {
    unsigned long long b = (items + WP_THREADS - 1) / WP_THREADS;
    return (int)(b < 1 ? 1 : (b > WP_MAX_BLOCKS ? WP_MAX_BLOCKS : b));
}

}  // namespace

hipError_t launch_wp_convert(int dt, const void* src, size_t count, float scale, bool scaled, bool out_bf16, void* dst, hipStream_t s) {
    if (dt < MME_DT_F32 || dt > MME_DT_F16 || count % 8 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    if (!count) return hipSuccess;
    ConvertArgs a{};
    a.src = src;
    a.chunks = count / 8;
    a.scale = scale;
    a.scaled = scaled;
    a.out_bf16 = out_bf16;
    a.dst = dst;
    const int grid = grid_for(a.chunks);
    if (dt == MME_DT_F32) convert_kernel<MME_DT_F32><<<grid, WP_THREADS, 0, s>>>(a);
    else if (dt == MME_DT_BF16) convert_kernel<MME_DT_BF16><<<grid, WP_THREADS, 0, s>>>(a);
    else convert_kernel<MME_DT_F16><<<grid, WP_THREADS, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_wp_pad(int dt, const void* src, int rows, int cols, int cols_padded, void* dst_bf16, hipStream_t s) {
    if (dt < MME_DT_F32 || dt > MME_DT_F16 || rows < 1 || cols < 4 || cols % 4 || cols_padded % 4 || cols_padded < cols || ((uintptr_t)src & 15))
        return hipErrorInvalidValue;
    const int grid = grid_for((unsigned long long)rows * (cols_padded / 4));
    if (dt == MME_DT_F32) pad_kernel<MME_DT_F32><<<grid, WP_THREADS, 0, s>>>(src, rows, cols, cols_padded, (uint16_t*)dst_bf16);
    else if (dt == MME_DT_BF16) pad_kernel<MME_DT_BF16><<<grid, WP_THREADS, 0, s>>>(src, rows, cols, cols_padded, (uint16_t*)dst_bf16);
    else pad_kernel<MME_DT_F16><<<grid, WP_THREADS, 0, s>>>(src, rows, cols, cols_padded, (uint16_t*)dst_bf16);
    return hipGetLastError();
}

hipError_t launch_wp_rowscale(int dt, const void* src, size_t rows, size_t cols, const void* factor, void* dst_bf16, hipStream_t s) {
    const size_t esz = dt == MME_DT_F32 ? 4 : 2;
    if (dt < MME_DT_F32 || dt > MME_DT_F16 || rows < 1 || cols < 8 || cols % 8 || ((uintptr_t)src & 15) || ((uintptr_t)dst_bf16 & 15) || !factor ||
        ((uintptr_t)factor % esz))
        return hipErrorInvalidValue;
    const unsigned long long chunks = (unsigned long long)rows * cols / 8;
    const int grid = grid_for(chunks);
    if (dt == MME_DT_F32) rowscale_kernel<MME_DT_F32><<<grid, WP_THREADS, 0, s>>>(src, chunks, cols, factor, dst_bf16);
    else if (dt == MME_DT_BF16) rowscale_kernel<MME_DT_BF16><<<grid, WP_THREADS, 0, s>>>(src, chunks, cols, factor, dst_bf16);
    else rowscale_kernel<MME_DT_F16><<<grid, WP_THREADS, 0, s>>>(src, chunks, cols, factor, dst_bf16);
    return hipGetLastError();
}

hipError_t launch_wp_mul(int dt, const void* src, const void* factor, size_t n, float* dst, hipStream_t s) {
    const size_t esz = dt == MME_DT_F32 ? 4 : 2;
    if (dt < MME_DT_F32 || dt > MME_DT_F16 || !src || !factor || !dst || ((uintptr_t)src % esz) || ((uintptr_t)factor % esz)) return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    const int grid = grid_for(n);
    if (dt == MME_DT_F32) mul_kernel<MME_DT_F32><<<grid, WP_THREADS, 0, s>>>(src, factor, n, dst);
    else if (dt == MME_DT_BF16) mul_kernel<MME_DT_BF16><<<grid, WP_THREADS, 0, s>>>(src, factor, n, dst);
    else mul_kernel<MME_DT_F16><<<grid, WP_THREADS, 0, s>>>(src, factor, n, dst);
    return hipGetLastError();
}

hipError_t launch_wp_fold(int dt, const WpFoldSrc* srcs, const size_t* rows, int nsrc, int cols, const void* gamma, const void* beta, void* wf, float* cs,
                          float* bf, hipStream_t s) {
    if (nsrc < 1 || nsrc > 3 || dt < MME_DT_F32 || dt > MME_DT_F16 || cols < FOLD_KT || cols % FOLD_KT || cols > FOLD_MAXK) return hipErrorInvalidValue;
    if (((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return hipErrorInvalidValue;
    FoldArgs a{};
    int total = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (rows[i] == 0 || rows[i] % FOLD_ROWS || ((uintptr_t)srcs[i].w & 15)) return hipErrorInvalidValue;
        a.src[i] = srcs[i];
        total += (int)rows[i];
        a.rows_end[i] = total;
    }
    a.nsrc = nsrc;
    a.cols = cols;
    a.gamma = gamma;
    a.beta = beta;
    a.wf = (uint16_t*)wf;
    a.cs = cs;
    a.bf = bf;
    const int grid = total / FOLD_ROWS;
    if (dt == MME_DT_F32) fold_kernel<MME_DT_F32><<<grid, FOLD_ROWS, 0, s>>>(a);
    else if (dt == MME_DT_BF16) fold_kernel<MME_DT_BF16><<<grid, FOLD_ROWS, 0, s>>>(a);
    else fold_kernel<MME_DT_F16><<<grid, FOLD_ROWS, 0, s>>>(a);
    return hipGetLastError();
}

extern "C" {

int mme_weights_fingerprint(mme_ctx* c, int cap, uint64_t* out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return fail(c, MME_E_ARG, "mme_weights_fingerprint: null argument or negative capacity");
    const int n = (int)c->allocs.size();
    if (n == 0 || cap == 0) return n;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    std::vector<FpBuf> h(n);
    for (int i = 0; i < n; ++i) h[i] = FpBuf{c->allocs[i], (unsigned long long)c->alloc_bytes[i]};
    void* ws = nullptr;
    const size_t tab = (size_t)n * sizeof(FpBuf), res = (size_t)n * sizeof(unsigned long long);
    hipError_t e = hipMalloc(&ws, tab + res);
    if (e != hipSuccess) return fail(c, MME_E_NOMEM, "mme_weights_fingerprint: hipMalloc: %s", hipGetErrorString(e));
    std::vector<unsigned long long> sums(n);
    e = hipMemcpy(ws, h.data(), tab, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset((char*)ws + tab, 0, res);
    if (e == hipSuccess) {
        fingerprint_kernel<<<dim3(FP_BLOCKS, n), WP_THREADS>>>((const FpBuf*)ws, (unsigned long long*)((char*)ws + tab));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(sums.data(), (char*)ws + tab, res, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (e != hipSuccess) return fail(c, MME_E_HIP, "mme_weights_fingerprint: %s", hipGetErrorString(e));
    for (int i = 0; i < n && i < cap; ++i) out[i] = sums[i];
    return n;
}

int64_t mme_weights_read(mme_ctx* c, int index, int64_t cap_bytes, void* dst_host) {
    if (!c) return MME_E_ARG;
    const int n = (int)c->allocs.size();
    if (index < 0 || index >= n) return fail(c, MME_E_ARG, "mme_weights_read: index %d outside 0..%d (the context holds %d prepared buffers)", index, n - 1, n);
    if (cap_bytes < 0 || (cap_bytes > 0 && !dst_host)) return fail(c, MME_E_ARG, "mme_weights_read: negative capacity, or a null destination with cap_bytes > 0");
    const size_t size = c->alloc_bytes[index], take = (size_t)cap_bytes < size ? (size_t)cap_bytes : size;
    if (take) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipMemcpy(dst_host, c->allocs[index], take, hipMemcpyDeviceToHost));
    }
    return (int64_t)size;
}

// ---- single launches of the preparation kernels on caller-owned buffers (tests/test_gpu_weight_prep.py): as
// mme_rowop_apply, every assumption of the launchers and kernels is checked here, so that a bad argument is an MME_E_ARG
// and never a launch
int mme_weight_prep_apply(mme_ctx* c, int op, const mme_weight_prep_apply_args* a, void* stream) {
    if (int r = hook_args(c, "mme_weight_prep_apply", a, op, 2)) return r;
    if (a->dtype < MME_DT_F32 || a->dtype > MME_DT_F16)
        return fail(c, MME_E_ARG, "mme_weight_prep_apply: dtype %d (MME_DT_F32 = 0, MME_DT_BF16 = 1, MME_DT_F16 = 2)", a->dtype);
    const size_t esz = a->dtype == MME_DT_F32 ? 4 : 2;
    const char* bad = nullptr;
    WpFoldSrc srcs[3] = {};
    size_t rows[3] = {0, 0, 0};
    switch (op) {
        case 0:
            if (a->count < 0 || a->count > ((int64_t)1 << 40) || (a->count % 8) != 0) bad = "0 <= count <= 2^40, count % 8 == 0";
            else if (!vec16(a->src) || !vec16(a->dst)) bad = "src, dst non-null and 16-byte aligned";
            break;
        case 1:
            if (a->rows < 1 || a->cols < 4 || (a->cols % 4) != 0 || (a->cols_padded % 4) != 0 || a->cols_padded < a->cols)
                bad = "rows >= 1, cols >= 4, cols % 4 == 0, cols_padded % 4 == 0, cols_padded >= cols";
            else if (!vec16(a->src) || !vec16(a->dst)) bad = "src, dst non-null and 16-byte aligned";
            break;
        default:
            if (a->nsrc < 1 || a->nsrc > 3) bad = "nsrc in 1..3";
            else if (a->cols < FOLD_KT || (a->cols % FOLD_KT) != 0 || a->cols > FOLD_MAXK) bad = "cols a multiple of 64, 64 <= cols <= 1280";
            else if (!vec16(a->gamma) || !vec16(a->beta) || !vec16(a->wf) || !vec16(a->cs) || !vec16(a->bf)) bad = "gamma, beta, wf, cs, bf non-null and 16-byte aligned";
            for (int i = 0; !bad && i < a->nsrc; ++i) {
                if (a->src_rows[i] < FOLD_ROWS || (a->src_rows[i] % FOLD_ROWS) != 0 || a->src_rows[i] > (1 << 24)) bad = "every rows[i] a non-zero multiple of 64, <= 2^24";
                else if (!vec16(a->w[i])) bad = "every w[i] non-null and 16-byte aligned";
                else if ((uintptr_t)a->b[i] % esz) bad = "every b[i] null or aligned to its element";
                srcs[i] = WpFoldSrc{a->w[i], a->b[i], a->src_scale[i], a->src_scaled[i] ? 1 : 0};
                rows[i] = (size_t)a->src_rows[i];
            }
            break;
    }
    if (bad) return fail(c, MME_E_ARG, "mme_weight_prep_apply: op %d needs %s", op, bad);
    if (op == 0 && a->count == 0) return MME_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    switch (op) {
        case 0: HIP_TRY(c, launch_wp_convert(a->dtype, a->src, (size_t)a->count, a->scale, a->scaled != 0, a->out_bf16 != 0, a->dst, s)); break;
        case 1: HIP_TRY(c, launch_wp_pad(a->dtype, a->src, a->rows, a->cols, a->cols_padded, a->dst, s)); break;
        default: HIP_TRY(c, launch_wp_fold(a->dtype, srcs, rows, a->nsrc, a->cols, a->gamma, a->beta, a->wf, a->cs, a->bf, s)); break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

}  // extern "C"
