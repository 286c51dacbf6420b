// K16: the silhouette of a partition of the L2-normalised bf16 vector table, without the N x N distance matrix.
//
// With d(i, j) = 1 - x_i . x_j the distances from row i to the members of cluster c add up to n_c - x_i . S_c, S_c the f64
// sum of the cluster's rows (what kmeans_update leaves in `sums`).  So every sample value follows from one skinny product
// g = X[N, d] . S[k, d]^T in f64 and a row-wise epilogue, O(N k d):
//   silhouette_rows   a workgroup of 256 owns 128 rows and walks the clusters in tiles of 64, streaming d in chunks of 16
//                     through LDS (the bf16 rows widened exactly to f64 on the way in).  Each thread keeps an 8 x 4 block of
//                     g in registers -- plain f64 FMAs, every g_ic one chain in ascending t -- and, per row, only the
//                     running minimum of 1 - g_ic' / n_c' over the foreign clusters with members; the one thread that meets
//                     the row's own cluster leaves that g in LDS.  q_i = sum x_it^2 rides along in the first tile.  Nothing of
//                     size [N, k] is written, so k is not bounded by memory.
//   sil_cluster_sums  one workgroup per cluster: thread t adds the samples at positions t, t + 256, ... of the cluster's part
//                     of `order` (ascending rows), then a fixed tree
//   sil_score         one workgroup: the same over the clusters' sums, the rows counted and the clusters with members
// No floating-point atomics: every output is bit-identical run to run.
#include "common.h"
#include "kmeans.h"

namespace {

constexpr int TM = 128, TK = 16;  // rows of a tile, columns of d per LDS chunk; a tile holds 16 * CJ clusters (CJ = 4 or 8)
constexpr int XP = TM + 2;        // padded LDS pitch (doubles; the clusters' is 16 * CJ + 2); keeps 16-byte alignment of 2-double reads

// 1 - g / n, the mean distance to a foreign cluster: a division, then a subtraction
__device__ __forceinline__ double foreign_mean(double g, int n) {
#pragma clang fp contract(off)
    const double m = g / (double)n;
    return 1.0 - m;
}

// the sample value from the own-cluster g, q = x . x, the own cluster's size and the least foreign mean, with exactly the
// operations of include/mme.h in their order
__device__ __forceinline__ double sample_value(double g, double q, int n, double b) {
#pragma clang fp contract(off)
    if (n == 1) return 0.0;
    const double nd = (double)n;
    const double within = nd - g;  // the distances to all members, the row itself among them
    const double self = 1.0 - q;   // the row's own, not exactly 0 on bf16 rows
    const double a = (within - self) / (nd - 1.0);
    const double s = (b - a) / fmax(a, b);
    return s != s ? 0.0 : s;
}

// what one thread brings in for a step (a chunk of TK columns of one cluster tile): 8 bf16 of its row, CJ f64 of its cluster
template <int CJ>
__device__ __forceinline__ void fetch_chunk(const uint16_t* x_src, bool x_in, const double* sums, int d, int k, int nchunk, int sc, int sq,
                                            int64_t step, uint4& px, double2 (&ps)[CJ / 2]) {
    const int tile = (int)(step / nchunk), t0 = (int)(step - (int64_t)tile * nchunk) * TK;
    px = x_in ? *(const uint4*)(x_src + t0) : make_uint4(0, 0, 0, 0);
    const int col = tile * 16 * CJ + sc;
    if (col < k) {
        const double2* src = (const double2*)(sums + (int64_t)col * d + t0 + sq);
#pragma unroll
        for (int u = 0; u < CJ / 2; ++u) ps[u] = src[u];
    } else {
#pragma unroll
        for (int u = 0; u < CJ / 2; ++u) ps[u] = make_double2(0.0, 0.0);
    }
}

template <int CJ>
__global__ __launch_bounds__(256) void silhouette_rows(const uint16_t* __restrict__ emb, int N, int d, const int32_t* __restrict__ label, int k,
                                                       const double* __restrict__ sums, const int32_t* __restrict__ counts,
                                                       double* __restrict__ sample) {
    __shared__ __attribute__((aligned(16))) double s_x[TK * XP];
    constexpr int TN = 16 * CJ, SP = TN + 2, TPC = 16 / CJ;  // clusters of a tile, their LDS pitch, threads that fetch one cluster's chunk
    constexpr int UNR = CJ == 4 ? 2 : 1;  // of the t loop: more hoists the LDS reads and runs out of registers (2 waves per SIMD want <= 256)
    __shared__ __attribute__((aligned(16))) double s_s[TK * SP];
    __shared__ double s_g[TM];
    __shared__ int s_lab[TM];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    if (tid < TM) {
        const int64_t row = row0 + tid;
        const int l = row < N ? label[row] : -1;
        s_lab[tid] = (unsigned)l < (unsigned)k ? l : -1;
        s_g[tid] = 0.0;
    }
    // what this thread brings in per chunk: 8 bf16 of one row, CJ f64 of one cluster
    const int xr = tid >> 1, xh = (tid & 1) * 8;
    const int sc = tid / TPC, sq = (tid % TPC) * CJ;
    const bool x_in = row0 + xr < N;
    const uint16_t* x_src = emb + (row0 + xr) * d + xh;
    const int nchunk = d / TK, ntile = (k + TN - 1) / TN;
    const int64_t steps = (int64_t)ntile * nchunk;
    uint4 px;
    double2 ps[CJ / 2];
    double acc[8][CJ], q[8], bmin[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        q[r] = 0.0;
        bmin[r] = __longlong_as_double(0x7ff0000000000000ll);  // +inf: no foreign cluster with members yet
#pragma unroll
        for (int j = 0; j < CJ; ++j) acc[r][j] = 0.0;
    }
    fetch_chunk<CJ>(x_src, x_in, sums, d, k, nchunk, sc, sq, 0, px, ps);
    for (int64_t step = 0; step < steps; ++step) {
        const int tile = (int)(step / nchunk), chunk = (int)(step - (int64_t)tile * nchunk);
        __syncthreads();  // the chunk before has been read (and, at step 0, s_lab and s_g are written)
        {
            const uint32_t w[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s_x[(xh + 2 * u) * XP + xr] = (double)__uint_as_float(w[u] << 16);
                s_x[(xh + 2 * u + 1) * XP + xr] = (double)__uint_as_float(w[u] & 0xffff0000u);
            }
#pragma unroll
            for (int u = 0; u < CJ / 2; ++u) {
                s_s[(sq + 2 * u) * SP + sc] = ps[u].x;
                s_s[(sq + 2 * u + 1) * SP + sc] = ps[u].y;
            }
        }
        __syncthreads();
        if (step + 1 < steps) fetch_chunk<CJ>(x_src, x_in, sums, d, k, nchunk, sc, sq, step + 1, px, ps);  // in flight during the FMAs below
#pragma unroll UNR
        for (int t = 0; t < TK; ++t) {
            double a[8], b[CJ];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double2 v = *(const double2*)(s_x + t * XP + ty * 8 + 2 * u);
                a[2 * u] = v.x;
                a[2 * u + 1] = v.y;
            }
#pragma unroll
            for (int u = 0; u < CJ / 2; ++u) {
                const double2 v = *(const double2*)(s_s + t * SP + tx * CJ + 2 * u);
                b[2 * u] = v.x;
                b[2 * u + 1] = v.y;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int j = 0; j < CJ; ++j) acc[r][j] = fma(a[r], b[j], acc[r][j]);
            if (tile == 0) {  // uniform
#pragma unroll
                for (int r = 0; r < 8; ++r) q[r] = fma(a[r], a[r], q[r]);
            }
        }
        if (chunk == nchunk - 1) {  // the tile's g is complete
            int n4[CJ];
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                const int col = tile * TN + tx * CJ + j;
                n4[j] = col < k ? counts[col] : 0;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int own = s_lab[ty * 8 + r];
#pragma unroll
                for (int j = 0; j < CJ; ++j) {
                    if (n4[j] > 0) {
                        if (tile * TN + tx * CJ + j == own) {
                            s_g[ty * 8 + r] = acc[r][j];  // one thread of one tile per row
                        } else {
                            const double m = foreign_mean(acc[r][j], n4[j]);
                            bmin[r] = m < bmin[r] ? m : bmin[r];
                        }
                    }
                    acc[r][j] = 0.0;
                }
            }
        }
    }
    // the 16 threads of a row group sit in 16 consecutive lanes
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const double other = __shfl_xor(bmin[r], o);
            bmin[r] = other < bmin[r] ? other : bmin[r];
        }
    __syncthreads();  // s_g
    if (tx == 0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t row = row0 + ty * 8 + r;
            if (row < N) {
                const int own = s_lab[ty * 8 + r];
                sample[row] = own < 0 ? __longlong_as_double(0x7ff8000000000000ll) : sample_value(s_g[ty * 8 + r], q[r], counts[own], bmin[r]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void sil_cluster_sums(const double* __restrict__ sample, const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ start, const int32_t* __restrict__ counts,
                                                        double* __restrict__ csum, double* __restrict__ cluster) {
#pragma clang fp contract(off)
    __shared__ double s_sum[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int n = counts[c];
    const int32_t* ord = order + start[c];
    double acc = 0.0;
    for (int p = t; p < n; p += 256) acc += sample[ord[p]];
    s_sum[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_sum[t] += s_sum[t + o];
        __syncthreads();
    }
    if (t == 0) {
        csum[c] = s_sum[0];
        cluster[c] = n > 0 ? s_sum[0] / (double)n : __longlong_as_double(0x7ff8000000000000ll);
    }
}

__global__ __launch_bounds__(1024) void sil_score(const double* __restrict__ csum, const int32_t* __restrict__ counts, int k,
                                                  double* __restrict__ score, long long* __restrict__ info) {
#pragma clang fp contract(off)
    __shared__ double s_sum[1024];
    __shared__ long long s_rows[1024];
    __shared__ int s_used[1024];
    const int t = threadIdx.x;
    double acc = 0.0;
    long long rows = 0;
    int used = 0;
    for (int c = t; c < k; c += 1024) {
        const int n = counts[c];
        if (n > 0) {  // an empty cluster's sum is 0 anyway
            acc += csum[c];
            rows += n;
            used += 1;
        }
    }
    s_sum[t] = acc;
    s_rows[t] = rows;
    s_used[t] = used;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            s_sum[t] += s_sum[t + o];
            s_rows[t] += s_rows[t + o];
            s_used[t] += s_used[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        info[0] = s_rows[0];
        info[1] = s_used[0];
        score[0] = s_used[0] >= 2 && s_rows[0] > 0 ? s_sum[0] / (double)s_rows[0] : __longlong_as_double(0x7ff8000000000000ll);
    }
}

}  // namespace

hipError_t launch_silhouette_rows(const uint16_t* emb, int N, int d, const int32_t* label, int k, const double* sums, const int32_t* counts,
                                  double* sample, hipStream_t s) {
    if (N < 1 || k < 1 || d < 64 || (d & 63) != 0 || ((uintptr_t)emb & 15) != 0 || ((uintptr_t)sums & 15) != 0) return hipErrorInvalidValue;
    // up to 64 clusters fit one narrow tile; beyond that the wide tile halves the LDS reads per FMA
    const dim3 grid((unsigned)((N + TM - 1) / TM));
    if (k <= 64)
        hipLaunchKernelGGL(silhouette_rows<4>, grid, dim3(256), 0, s, emb, N, d, label, k, sums, counts, sample);
    else
        hipLaunchKernelGGL(silhouette_rows<8>, grid, dim3(256), 0, s, emb, N, d, label, k, sums, counts, sample);
    return hipGetLastError();
}

hipError_t launch_silhouette_reduce(const double* sample, const int32_t* order, const int32_t* start, const int32_t* counts, int k, double* csum,
                                    double* cluster, double* score, long long* info, hipStream_t s) {
    if (k < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sil_cluster_sums, dim3(k), dim3(256), 0, s, sample, order, start, counts, csum, cluster);
    hipLaunchKernelGGL(sil_score, dim3(1), dim3(1024), 0, s, csum, counts, k, score, info);
    return hipGetLastError();
}
