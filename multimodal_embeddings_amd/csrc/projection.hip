// K17: the moments of the bf16 vector table and the projection of its rows (include/mme.h).
//
// Moments (K17a).  The column sums and the d x d second-moment matrix contract over the ROWS of the table, in f64, in an
// order that is part of the definition: the rows are cut into blocks of MME_MOMENTS_BLOCK, every element of a block's
// partial is ONE chain of f64 fused multiply-adds over the block's rows in ascending order (a product of two bf16 values
// is exact in f64, so the fma is the multiply-then-add of the restatement), and the partials are added in ascending block
// order.  No floating-point atomics, no tree whose shape depends on the grid: bit-identical run to run.
//   moments_block   one workgroup per (upper-triangle pair of 64-column tiles, row block): 256 lanes, a 4 x 4 register tile of
//                   f64 accumulators each; the block's rows go through LDS 32 at a time, widened to f64 once.  The workgroups
//                   of the diagonal tiles also leave the block's column sums.
//   moments_reduce  one lane per element of the upper triangle: the partials in ascending block order on top of +0.0 (or of
//                   what the block group before left), stored at [a, c] and at [c, a].
// Projection (K17b).  project_rows is a tiled f32 kernel: 128 rows x 128 components per workgroup, 8 x 8 per lane (128 x 64,
// 8 x 4, when m <= 64), the centred rows (f32(x) - mean, one rounding) and the weights through LDS 32 columns at a time, one
// fused multiply-add per product, two of them per v_pk_fma_f32.
// Consecutive workgroups walk the component tiles of one row tile, so the rows are read from HBM once; the weights (4 MiB at
// the most) stay in L2.
#include "common.h"
#include "projection.h"

namespace {

constexpr int MB_SLAB = 32;  // rows of a block in LDS at a time: 2 x 32 x 64 f64 = 32 KiB

__device__ __forceinline__ void pair_tiles(int pair, int T, int& ta, int& tc) {
    int a = 0;
    while (pair >= T - a) {  // T <= 16
        pair -= T - a;
        ++a;
    }
    ta = a;
    tc = a + pair;
}

__device__ __forceinline__ void widen8(const uint4 v, double* dst) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        dst[2 * u] = (double)__uint_as_float(w[u] << 16);
        dst[2 * u + 1] = (double)__uint_as_float(w[u] & 0xffff0000u);
    }
}

template <int ROWS>
__device__ __forceinline__ void moments_rows(const double (*sa)[PJ_TILE], const double (*sc)[PJ_TILE], int n, int ty, int tx, double (&acc)[4][4]) {
    // ROWS > 0: a whole slab, unrolled; ROWS == 0: the n rows of the block's last slab
    const int rows = ROWS ? ROWS : n;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
        double a[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sa[r][4 * ty + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = sc[r][4 * tx + u];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], c[v], acc[u][v]);
    }
}

// grid (pairs, blocks of the group)
__global__ __launch_bounds__(256) void moments_block(const uint16_t* __restrict__ emb, int64_t N, int d, int64_t b0, double* __restrict__ part,
                                                     double* __restrict__ psum) {
    __shared__ __attribute__((aligned(16))) double s_a[MB_SLAB][PJ_TILE];
    __shared__ __attribute__((aligned(16))) double s_c[MB_SLAB][PJ_TILE];
    int ta, tc;
    pair_tiles(blockIdx.x, d / PJ_TILE, ta, tc);
    const bool diag = ta == tc;
    const int64_t row0 = (b0 + blockIdx.y) * MME_MOMENTS_BLOCK;
    const int nrows = (int)min((int64_t)MME_MOMENTS_BLOCK, N - row0);  // >= 1: the launcher counts the blocks
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int lr = t >> 3, lc = (t & 7) * 8;  // the 8 values this lane brings in: row lr of the slab, columns lc .. lc + 7 of a tile
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    double ps = 0.0;
    const double(*sc)[PJ_TILE] = diag ? s_a : s_c;
    for (int r0 = 0; r0 < nrows; r0 += MB_SLAB) {
        const int n = min(MB_SLAB, nrows - r0);
        __syncthreads();  // the slab before has been consumed
        if (lr < n) {
            const uint16_t* src = emb + (row0 + r0 + lr) * d + lc;
            widen8(*(const uint4*)(src + ta * PJ_TILE), &s_a[lr][lc]);
            if (!diag) widen8(*(const uint4*)(src + tc * PJ_TILE), &s_c[lr][lc]);
        }
        __syncthreads();
        if (n == MB_SLAB)
            moments_rows<MB_SLAB>(s_a, sc, n, ty, tx, acc);
        else
            moments_rows<0>(s_a, sc, n, ty, tx, acc);
        if (diag && t < PJ_TILE)  // wave 0
            for (int r = 0; r < n; ++r) ps += s_a[r][t];
    }
    double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (PJ_TILE * PJ_TILE);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(4 * ty + u) * PJ_TILE + 4 * tx + v] = acc[u][v];
    if (diag && t < PJ_TILE) psum[(size_t)blockIdx.y * d + ta * PJ_TILE + t] = ps;
}

// workgroups 0 .. 16 pairs - 1: 256 elements of a tile each; the rest: 256 columns of the sums each
__global__ __launch_bounds__(256) void moments_reduce(const double* __restrict__ part, const double* __restrict__ psum, int nb, int d, int pairs, int first,
                                                      double* __restrict__ sum, double* __restrict__ gram) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < pairs * 16) {
        const int pair = blockIdx.x >> 4, e = (blockIdx.x & 15) * 256 + t;
        int ta, tc;
        pair_tiles(pair, d / PJ_TILE, ta, tc);
        const int a = ta * PJ_TILE + (e >> 6), c = tc * PJ_TILE + (e & 63);
        const size_t per = (size_t)pairs * (PJ_TILE * PJ_TILE);
        const double* p = part + (size_t)pair * (PJ_TILE * PJ_TILE) + e;
        double acc = first ? 0.0 : gram[(size_t)a * d + c];
        int b = 0;
        for (; b + 8 <= nb; b += 8) {  // 8 loads in flight, added in order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(b + u) * per];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; b < nb; ++b) acc += p[(size_t)b * per];
        gram[(size_t)a * d + c] = acc;
        if (ta != tc) gram[(size_t)c * d + a] = acc;  // a diagonal tile holds both halves already, bit-equal: the products commute
    } else {
        const int c = ((int)blockIdx.x - pairs * 16) * 256 + t;
        if (c >= d) return;
        double acc = first ? 0.0 : sum[c];
        for (int b = 0; b < nb; ++b) acc += psum[(size_t)b * d + c];
        sum[c] = acc;
    }
}

constexpr int PR_K = 32;     // columns of d in LDS at a time
constexpr int PR_ROWS = 128;  // rows of a tile: 8 per lane, 4 at 4 * ty and 4 at 64 + 4 * ty
typedef __attribute__((ext_vector_type(2))) float f32x2;

// TN components per tile (64 or 128): TN / 16 per lane, 4 at 4 * tx and, for TN = 128, 4 more at 64 + 4 * tx, so that every
// ds_read_b128 of a wave covers one contiguous run.  The products go pairwise through v_pk_fma_f32: one fused multiply-add
// per element, as fmaf.
template <int TN>
__global__ __launch_bounds__(256) void project_rows(const uint16_t* __restrict__ emb, int64_t rows, int d, const float* __restrict__ mean,
                                                    const float* __restrict__ w, int m, int jtiles, float* __restrict__ y0, int64_t ld0,
                                                    float* __restrict__ y1, int64_t ld1) {
    constexpr int CH = TN / 64;          // halves of 64 components
    constexpr int WV = TN * PR_K / 256;  // weight values a lane brings in per slab: 8 or 16
    __shared__ __attribute__((aligned(16))) float s_x[PR_K][PR_ROWS + 4];  // [column of d][row of the tile]: f32(x) - mean
    __shared__ __attribute__((aligned(16))) float s_w[PR_K][TN + 4];       // [column of d][component of the tile]
    const int64_t i0 = (int64_t)(blockIdx.x / jtiles) * PR_ROWS;
    const int j0 = (int)(blockIdx.x % jtiles) * TN;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int xr = t >> 1, xc = (t & 1) * 16;            // rows: columns xc .. xc + 15 of row xr
    const int wr = t / (PR_K / WV), wc = (t % (PR_K / WV)) * WV;  // weights: columns wc .. wc + WV - 1 of component wr
    const bool row_ok = i0 + xr < rows, w_ok = j0 + wr < m;
    const uint16_t* xsrc = emb + (i0 + xr) * d + xc;
    const float* wsrc = w + (size_t)(j0 + wr) * d + wc;
    f32x2 acc[8][2 * CH];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 2 * CH; ++v) acc[u][v] = f32x2{0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += PR_K) {
        float xv[16], wv[WV];
        if (row_ok) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 q = *(const uint4*)(xsrc + k0 + 8 * h);
                const f32x4 m0 = *(const f32x4*)(mean + k0 + xc + 8 * h), m1 = *(const f32x4*)(mean + k0 + xc + 8 * h + 4);
                const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xv[8 * h + 2 * u] = __uint_as_float(qq[u] << 16);
                    xv[8 * h + 2 * u + 1] = __uint_as_float(qq[u] & 0xffff0000u);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xv[8 * h + u] -= m0[u];
                    xv[8 * h + 4 + u] -= m1[u];
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) xv[u] = 0.f;
        }
        if (w_ok) {
#pragma unroll
            for (int h = 0; h < WV / 4; ++h) {
                const f32x4 q = *(const f32x4*)(wsrc + k0 + 4 * h);
#pragma unroll
                for (int u = 0; u < 4; ++u) wv[4 * h + u] = q[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < WV; ++u) wv[u] = 0.f;
        }
        __syncthreads();  // the slab before has been consumed
#pragma unroll
        for (int u = 0; u < 16; ++u) s_x[xc + u][xr] = xv[u];
#pragma unroll
        for (int u = 0; u < WV; ++u) s_w[wc + u][wr] = wv[u];
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < PR_K; ++c) {
            float a[8];
            f32x2 b[2 * CH];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 q = *(const f32x4*)&s_x[c][64 * h + 4 * ty];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[4 * h + u] = q[u];
            }
#pragma unroll
            for (int h = 0; h < CH; ++h) {
                const f32x4 q = *(const f32x4*)&s_w[c][64 * h + 4 * tx];
                b[2 * h] = f32x2{q[0], q[1]};
                b[2 * h + 1] = f32x2{q[2], q[3]};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int v = 0; v < 2 * CH; ++v) acc[u][v] = __builtin_elementwise_fma(f32x2{a[u], a[u]}, b[v], acc[u][v]);
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t i = i0 + 64 * (u >> 2) + 4 * ty + (u & 3);
        if (i >= rows) continue;
#pragma unroll
        for (int h = 0; h < CH; ++h) {
            const int j = j0 + 64 * h + 4 * tx;
            if (j >= m) continue;
            const f32x2 lo = acc[u][2 * h], hi = acc[u][2 * h + 1];
            const float v4[4] = {lo[0], lo[1], hi[0], hi[1]};
            float* dst[2] = {y0 ? y0 + i * ld0 + j : nullptr, y1 ? y1 + i * ld1 + j : nullptr};
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                if (!dst[o]) continue;
                if (j + 3 < m) {
                    *(f32x4*)dst[o] = f32x4{v4[0], v4[1], v4[2], v4[3]};
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        if (j + v < m) dst[o][v] = v4[v];
                }
            }
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t launch_moments_block(const uint16_t* emb, int64_t N, int d, int64_t b0, int nb, double* part, double* psum, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    const int64_t blocks = (N + MME_MOMENTS_BLOCK - 1) / MME_MOMENTS_BLOCK;
    if (N < 1 || d < PJ_TILE || d > 1024 || (d % PJ_TILE) != 0 || b0 < 0 || nb > 65535 || b0 + nb > blocks || !emb || !aligned16(emb) || !part || !psum)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(moments_block, dim3((unsigned)moments_pairs(d), (unsigned)nb), dim3(256), 0, s, emb, N, d, b0, part, psum);
    return hipGetLastError();
}

hipError_t launch_moments_reduce(const double* part, const double* psum, int nb, int d, int first, double* sum, double* gram, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (d < PJ_TILE || d > 1024 || (d % PJ_TILE) != 0 || !part || !psum || !sum || !gram) return hipErrorInvalidValue;
    const int pairs = moments_pairs(d);
    hipLaunchKernelGGL(moments_reduce, dim3((unsigned)(pairs * 16 + (d + 255) / 256)), dim3(256), 0, s, part, psum, nb, d, pairs, first, sum, gram);
    return hipGetLastError();
}

hipError_t launch_project_rows(const uint16_t* emb, int64_t rows, int d, const float* mean, const float* w, int m, float* y0, int64_t ld0, float* y1,
                               int64_t ld1, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (rows > ((int64_t)1 << 24) || d < 64 || d > 65536 || (d % 64) != 0 || m < 1 || m > d || (!y0 && !y1)) return hipErrorInvalidValue;
    if (!emb || !mean || !w || !aligned16(emb) || !aligned16(mean) || !aligned16(w) || !aligned16(y0) || !aligned16(y1)) return hipErrorInvalidValue;
    if ((y0 && (ld0 < m || (ld0 & 3) != 0)) || (y1 && (ld1 < m || (ld1 & 3) != 0))) return hipErrorInvalidValue;
    const int64_t itiles = (rows + PR_ROWS - 1) / PR_ROWS;  // <= 2^17, times at most 2^10 component tiles
    if (m <= 64) {
        hipLaunchKernelGGL(project_rows<64>, dim3((unsigned)itiles), dim3(256), 0, s, emb, rows, d, mean, w, m, 1, y0, ld0, y1, ld1);
    } else {
        const int jtiles = (m + 127) / 128;
        hipLaunchKernelGGL(project_rows<128>, dim3((unsigned)(itiles * jtiles)), dim3(256), 0, s, emb, rows, d, mean, w, m, jtiles, y0, ld0, y1, ld1);
    }
    return hipGetLastError();
}
