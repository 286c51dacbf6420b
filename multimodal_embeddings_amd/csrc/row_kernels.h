// Device-side pieces of the row kernels (rowops.hip, text_tower.hip): one 64-lane wave owns one row of D values.  Every
// tower's LayerNorm row, pooled row and L2 step is built from these, so they cannot drift apart: the two-pass f32
// LayerNorm (mean, then centred variance -- the form torch's LayerNorm uses, transformers modeling_vit.py:261-262,348) and
// torch.nn.functional.normalize's x / max(||x||_2, 1e-12) are each written here once.
#pragma once
#include "common.h"

// a row of D values over 64 lanes: NT accesses of V consecutive values per lane, access t at column t * 64 V + lane * V.
// 768 = 3 x 4 values per lane, 1024 = 4 x 4, 512 = 2 x 4 (the text width), 384 = 3 x 2 (4-byte accesses: 384 is no multiple
// of the 256 values a wave covers with 8-byte ones)
template <int D> struct RowShape {
    static_assert(D == 384 || D == 512 || D == 768 || D == 1024, "row kernels: widths 384, 512, 768 and 1024");
    static constexpr int V = (D % 256) == 0 ? 4 : 2;
    static constexpr int NT = D / (64 * V);
    typedef __attribute__((ext_vector_type(V))) __bf16 bvec;
    typedef __attribute__((ext_vector_type(V))) float fvec;
};

// the bf16 row as its lanes load it, not yet widened: NT independent loads (a kernel that wants several rows in flight issues
// these for all of them before it widens the first)
template <int D> __device__ __forceinline__ void row_load_raw(const bf16_t* xr, int lane, typename RowShape<D>::bvec (&p)[RowShape<D>::NT]) {
    typedef RowShape<D> RS;
#pragma unroll
    for (int t = 0; t < RS::NT; ++t) p[t] = *(const typename RS::bvec*)(xr + t * 64 * RS::V + lane * RS::V);
}
// p[] -> v[]: v[t * V + j] is column t * 64 V + lane * V + j
template <int D> __device__ __forceinline__ void row_widen(const typename RowShape<D>::bvec (&p)[RowShape<D>::NT], float (&v)[D / 64]) {
    typedef RowShape<D> RS;
#pragma unroll
    for (int t = 0; t < RS::NT; ++t) {
#pragma unroll
        for (int j = 0; j < RS::V; ++j) v[t * RS::V + j] = (float)p[t][j];
    }
}

// bf16 row -> v[]: v[t * V + j] is column t * 64 V + lane * V + j
template <int D> __device__ __forceinline__ void row_load(const bf16_t* xr, int lane, float (&v)[D / 64]) {
    typename RowShape<D>::bvec p[RowShape<D>::NT];
    row_load_raw<D>(xr, lane, p);
    row_widen<D>(p, v);
}

// (mean, rstd) of the row in v[], which stays as it is: two wave reductions, the sums over v[0..] ascending
template <int D> __device__ __forceinline__ float2 row_stats(const float (&v)[D / 64], float eps) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D / 64; ++j) s += v[j];
    const float mean = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < D / 64; ++j) {
        const float d = v[j] - mean;
        q += d * d;
    }
    return make_float2(mean, rsqrtf(wave_sum(q) * (1.0f / D) + eps));
}

// LayerNorm of the row already in v[] (row_load's layout): v[] leaves normalised, scaled and shifted, in f32
template <int D>
__device__ __forceinline__ void ln_apply(const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int lane, float (&v)[D / 64]) {
    typedef RowShape<D> RS;
    const float2 st = row_stats<D>(v, eps);
#pragma unroll
    for (int t = 0; t < RS::NT; ++t) {
        const int c = t * 64 * RS::V + lane * RS::V;
        const typename RS::fvec gv = *(const typename RS::fvec*)(gamma + c);
        const typename RS::fvec bv = *(const typename RS::fvec*)(beta + c);
#pragma unroll
        for (int j = 0; j < RS::V; ++j) v[t * RS::V + j] = (v[t * RS::V + j] - st.x) * st.y * gv[j] + bv[j];
    }
}

// LayerNorm of the bf16 row xr: v[] leaves normalised, scaled and shifted, in f32
template <int D>
__device__ __forceinline__ void ln_row(const bf16_t* xr, const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int lane,
                                       float (&v)[D / 64]) {
    row_load<D>(xr, lane, v);
    ln_apply<D>(gamma, beta, eps, lane, v);
}

// v[] -> bf16 row, one rounding to nearest even per value
template <int D> __device__ __forceinline__ void row_store_bf16(bf16_t* yr, int lane, const float (&v)[D / 64]) {
    typedef RowShape<D> RS;
#pragma unroll
    for (int t = 0; t < RS::NT; ++t) {
        typename RS::bvec o;
#pragma unroll
        for (int j = 0; j < RS::V; ++j) o[j] = (bf16_t)v[t * RS::V + j];
        *(typename RS::bvec*)(yr + t * 64 * RS::V + lane * RS::V) = o;
    }
}

// this lane's share of ||v||^2, summed over v[0..] ascending
template <int D> __device__ __forceinline__ float row_sumsq(const float (&v)[D / 64]) {
    float n2 = 0.f;
#pragma unroll
    for (int j = 0; j < D / 64; ++j) n2 += v[j] * v[j];
    return n2;
}

// 1 / max(||v||_2, 1e-12) from the wave's sum of squares
__device__ __forceinline__ float l2_inverse(float n2) { return 1.0f / fmaxf(sqrtf(n2), 1e-12f); }

// v * inv -> the row at element `off` of yf (f32) and / or yb (bf16; either may be null), the bf16 value the rounding of the
// f32 one.  A row narrower than D (`cols`, a multiple of 64, RowShape<1024> only): nothing is stored at the columns >= cols.
template <int D>
__device__ __forceinline__ void row_scale_store(const float (&v)[D / 64], float inv, int lane, float* yf, bf16_t* yb, int64_t off, int cols = D) {
    typedef RowShape<D> RS;
#pragma unroll
    for (int t = 0; t < RS::NT; ++t) {
        const int c = t * 64 * RS::V + lane * RS::V;
        if (c >= cols) continue;
        typename RS::fvec o;
        typename RS::bvec ob;
#pragma unroll
        for (int j = 0; j < RS::V; ++j) {
            o[j] = v[t * RS::V + j] * inv;
            ob[j] = (bf16_t)o[j];
        }
        if (yf) *(typename RS::fvec*)(yf + off + c) = o;
        if (yb) *(typename RS::bvec*)(yb + off + c) = ob;
    }
}

// The L2 step: v / max(||v||_2, 1e-12) -> the row at element `off` of yf / yb (row_scale_store).  n2 sums over v[0..]
// ascending.  A row narrower than D holds zeros at the columns >= cols.
template <int D>
__device__ __forceinline__ void row_l2_store(const float (&v)[D / 64], int lane, float* yf, bf16_t* yb, int64_t off, int cols = D) {
    row_scale_store<D>(v, l2_inverse(wave_sum(row_sumsq<D>(v))), lane, yf, yb, off, cols);
}

// launches the instantiation of a row kernel for width d; a width without one is an error, never another kernel.  The
// launchers admit the widths of their path first (common.h: vit_width_built 384 / 768 / 1024, text_width_built 512 / 768 / 1024).
#define ROW_KERNEL_BY_WIDTH(d, kernel, grid, s, ...)                                                          \
    switch (d) {                                                                                              \
        case 384: hipLaunchKernelGGL(kernel<384>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 512: hipLaunchKernelGGL(kernel<512>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 768: hipLaunchKernelGGL(kernel<768>, grid, dim3(256), 0, s, __VA_ARGS__); break;                 \
        case 1024: hipLaunchKernelGGL(kernel<1024>, grid, dim3(256), 0, s, __VA_ARGS__); break;               \
        default: return hipErrorInvalidValue;                                                                 \
    }
