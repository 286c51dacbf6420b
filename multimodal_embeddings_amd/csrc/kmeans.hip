// K15: spherical k-means over the L2-normalised bf16 vector table -- the kernels around the cosine GEMM.
//
// Assignment: the GEMM (EPI_F32) leaves the cosine of a chunk of rows against the k centroids as a block [rows, ld];
// `kmeans_argmax_rows` streams it once, ONE WAVE PER ROW (as topk_rows of K12).  Every value becomes a 64-bit key -- the
// order-preserving image of the f32 in the high word (0 for a NaN, which is below the image of -inf), 0xffffffff - column
// in the low word -- and the wave takes the maximum: a total order, so the winner does not depend on which lane saw what.
// The rows whose label changed are counted per workgroup and added with one integer atomic.
//
// Update: the sums must not depend on the schedule, so the rows of a cluster are brought together first and then added
// in ascending row order by ONE lane per (cluster, column) in f64 -- no floating-point atomics anywhere.  The grouping is
// a counting sort that is stable by construction, without any workgroup looking at all N labels:
//   km_rank        one workgroup per chunk of rows: the chunk's labels in LDS, rank[i] = rows of i's cluster before i
//                  inside the chunk, cnt[j, chunk] = rows of cluster j in the chunk
//   km_chunk_scan  one wave per cluster: cnt[j, .] becomes its exclusive prefix over the chunks, counts[j] the total
//   km_starts      one workgroup: start[j] = exclusive prefix of counts
//   km_scatter     order[start[j] + cnt[j, chunk] + rank[i]] = i  -- ascending i inside every cluster
//   km_sum         one wave per (cluster, 64-column slice) walks its part of `order`
//   km_centroid    one workgroup per cluster: n2 = sum of squares in ascending column order, one f64 -> bf16 rounding
// Every launch takes `run_if` and returns at once when *run_if == 0 (uniform), which is how mme_kmeans stops on the device.
#include "common.h"
#include "kmeans.h"

namespace {

__device__ __forceinline__ bool gate_closed(const int* run_if) { return run_if && *(const volatile int*)run_if == 0; }

__device__ __forceinline__ unsigned long long argmax_key(float v, int col) {
    const uint32_t u = __float_as_uint(v);
    uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if ((u & 0x7fffffffu) > 0x7f800000u) o = 0;  // NaN: below -inf, whose image is 0x007fffff
    return ((unsigned long long)o << 32) | (0xffffffffu - (uint32_t)col);
}

__global__ __launch_bounds__(256) void kmeans_argmax_rows(const float* __restrict__ qsim, int64_t ld, int k, int rows, int32_t* __restrict__ label,
                                                          float* __restrict__ sim, long long* __restrict__ moved, const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;  // uniform: every wave of every workgroup takes the same way
    __shared__ int s_moved[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    int mv = 0;
    if (row < rows) {  // whole wave
        const float* src = qsim + (int64_t)row * ld;
        unsigned long long best = 0;  // below every key
        // rows start 16-byte aligned (ld % 4 == 0): 4 consecutive values per lane, 1 KiB per wave step
        for (int j = 4 * lane; j < k; j += 256) {
            float e[4];
            if (j + 3 < k) {
                const float4 v = *(const float4*)(src + j);
                e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) e[t] = j + t < k ? src[j + t] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned long long key = argmax_key(e[t], j + t);
                if (j + t < k && key > best) best = key;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            if (other > best) best = other;
        }
        if (lane == 0) {
            const int col = (int)(0xffffffffu - (uint32_t)best);  // k >= 1: lane 0 holds column 0 at least
            mv = label[row] != col;
            label[row] = col;
            sim[row] = src[col];
        }
    }
    if (lane == 0) s_moved[w] = mv;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = s_moved[0] + s_moved[1] + s_moved[2] + s_moved[3];
        if (n) (void)__hip_atomic_fetch_add(moved, (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void km_zero(int32_t* __restrict__ p, int64_t n, const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0;
}

// dynamic LDS: int[chunk]
__global__ __launch_bounds__(256) void km_rank(const int32_t* __restrict__ label, int N, int k, int chunk, int32_t* __restrict__ rank,
                                               int32_t* __restrict__ cnt, const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    extern __shared__ int s_lab[];
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int n = (int)min((int64_t)chunk, (int64_t)N - r0);
    for (int q = threadIdx.x; q < n; q += 256) s_lab[q] = label[r0 + q];
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += 256) {
        const int l = s_lab[r];
        if ((unsigned)l >= (unsigned)k) {  // belongs to no cluster
            rank[r0 + r] = -1;
            continue;
        }
        int before = 0, total = 0;
        for (int q = 0; q < n; ++q) {  // all lanes read one address: a broadcast
            const int same = s_lab[q] == l;
            total += same;
            before += same & (q < r);
        }
        rank[r0 + r] = before;
        if (before == 0) cnt[(int64_t)l * gridDim.x + blockIdx.x] = total;  // the cluster's first row of the chunk writes for all
    }
}

// one wave per cluster: its row of cnt becomes the exclusive prefix over the chunks, 64 chunks per step
__global__ __launch_bounds__(256) void km_chunk_scan(int32_t* __restrict__ cnt, int nchunks, int k, int32_t* __restrict__ counts,
                                                     const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;  // whole wave
    int32_t* row = cnt + (int64_t)j * nchunks;
    int run = 0;
    for (int c0 = 0; c0 < nchunks; c0 += 64) {
        const int c = c0 + lane;
        const int v = c < nchunks ? row[c] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (c < nchunks) row[c] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) counts[j] = run;
}

// one workgroup of 1024: thread t owns the clusters [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void km_starts(const int32_t* __restrict__ counts, int k, int32_t* __restrict__ start, const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    __shared__ int s_part[1024];
    const int t = threadIdx.x;
    const int per = (k + 1023) / 1024;
    const int lo = min(t * per, k), hi = min(lo + per, k);
    int sum = 0;
    for (int j = lo; j < hi; ++j) sum += counts[j];
    s_part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan
        const int v = t >= o ? s_part[t - o] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;
    for (int j = lo; j < hi; ++j) {
        start[j] = run;
        run += counts[j];
    }
}

__global__ __launch_bounds__(256) void km_scatter(const int32_t* __restrict__ label, int N, int k, int chunk, int nchunks, const int32_t* __restrict__ rank,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ start, int32_t* __restrict__ order,
                                                  const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int l = label[i];
    if ((unsigned)l >= (unsigned)k) return;
    const int64_t pos = (int64_t)start[l] + cnt[(int64_t)l * nchunks + i / chunk] + rank[i];
    if (pos < N) order[pos] = (int32_t)i;  // always, while the labels are those km_rank read
}

// one wave per (cluster, 64 columns): the adds of a column happen in one lane, in ascending row order
__global__ __launch_bounds__(64) void km_sum(const uint16_t* __restrict__ emb, int N, int d, int k, const int32_t* __restrict__ order,
                                             const int32_t* __restrict__ start, const int32_t* __restrict__ counts, double* __restrict__ sums,
                                             const int* __restrict__ run_if) {
    if (gate_closed(run_if)) return;
    const int slices = d >> 6;
    const int j = blockIdx.x / slices, c = (blockIdx.x - j * slices) * 64 + threadIdx.x;
    const int n = counts[j];
    const int32_t* ord = order + start[j];
    double acc = 0.0;
    int p = 0;
    for (; p + 32 <= n; p += 32) {  // 32 rows in flight, added in order: a cluster of a thousand rows is a chain of loads otherwise
        uint16_t v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = emb[(int64_t)ord[p + u] * d + c];
#pragma unroll
        for (int u = 0; u < 32; ++u) acc += (double)bf16_bits_to_f32(v[u]);
    }
    for (; p + 8 <= n; p += 8) {
        uint16_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = emb[(int64_t)ord[p + u] * d + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)bf16_bits_to_f32(v[u]);
    }
    for (; p < n; ++p) acc += (double)bf16_bits_to_f32(emb[(int64_t)ord[p] * d + c]);
    sums[(int64_t)j * d + c] = acc;
}

// f64 -> bf16, one rounding to nearest even: to f32 toward zero with the lost bits kept as a sticky last bit (round to
// odd; f32 carries 16 bits more than bf16, so the second rounding sees exactly what the first dropped), then nearest even
__device__ __forceinline__ uint16_t f64_to_bf16_rne(double x) {
    const float f = __double2float_rz(x);
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    if ((double)f != x) u |= 1u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

__global__ __launch_bounds__(256) void km_centroid(const double* __restrict__ sums, const int32_t* __restrict__ counts, int d,
                                                   uint16_t* __restrict__ centroids, int lds, const int* __restrict__ run_if) {
#pragma clang fp contract(off)  // s * s is rounded before it is added: what the float64 restatement does
    if (gate_closed(run_if)) return;
    const int j = blockIdx.x;
    if (counts[j] == 0) return;  // an empty cluster keeps its centroid
    __shared__ double s_den;
    extern __shared__ double s_row[];  // [d] when lds != 0
    const double* row = sums + (int64_t)j * d;
    if (lds) {
        for (int c = threadIdx.x; c < d; c += 256) s_row[c] = row[c];
        __syncthreads();
    }
    if (threadIdx.x == 0) {  // one lane, ascending c: the order is the definition
        const double* src = lds ? s_row : row;
        double n2 = 0.0;
        for (int c = 0; c < d; c += 8) {  // d % 64 == 0
            double s[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] = src[c + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double sq = s[u] * s[u];
                n2 = n2 + sq;
            }
        }
        const double nrm = __dsqrt_rn(n2);
        s_den = nrm > 1e-12 ? nrm : 1e-12;
    }
    __syncthreads();
    const double den = s_den;
    for (int c = threadIdx.x; c < d; c += 256) centroids[(int64_t)j * d + c] = f64_to_bf16_rne(row[c] / den);
}

__global__ __launch_bounds__(1024) void kmeans_step_end(int* __restrict__ ctrl, long long* __restrict__ moved, const float* __restrict__ sim, int N,
                                                        const int32_t* __restrict__ counts, int k, long long* __restrict__ info,
                                                        double* __restrict__ objective, int first) {
    const int go = first ? 1 : *(const volatile int*)ctrl;
    if (!go) return;  // uniform; nobody has written ctrl yet
    __shared__ double s_sum[1024];
    __shared__ int s_empty[1024];
    const int t = threadIdx.x;
    // a fixed order: thread t adds sim[t], sim[t + 1024], ... in f64, then a tree over the 1024 partial sums
    double acc = 0.0;
#pragma unroll 8
    for (int i = t; i < N; i += 1024) acc += (double)sim[i];
    int empty = 0;
    if (!first)
        for (int j = t; j < k; j += 1024) empty += counts[j] == 0;
    s_sum[t] = acc;
    s_empty[t] = empty;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            s_sum[t] += s_sum[t + o];
            s_empty[t] += s_empty[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        objective[0] = s_sum[0];
        if (first) {
            ctrl[0] = 1;
            info[0] = info[1] = info[2] = info[3] = 0;
        } else {
            const long long mv = *moved;
            info[0] += 1;
            info[1] = mv;
            info[2] = mv == 0;
            info[3] = s_empty[0];
            ctrl[0] = mv != 0;
        }
        *moved = 0;
    }
}

__global__ __launch_bounds__(256) void km_fill_labels(int32_t* __restrict__ labels, int N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) labels[i] = -1;
}

// one thread per 16 bytes
__global__ __launch_bounds__(256) void km_gather_rows(const uint16_t* __restrict__ src, const int32_t* __restrict__ rows, int k, int d,
                                                      uint16_t* __restrict__ dst) {
    const int per = d >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)k * per) return;
    const int j = (int)(i / per), v = (int)(i - (int64_t)j * per);
    ((uint4*)(dst + (int64_t)j * d))[v] = ((const uint4*)(src + (int64_t)rows[j] * d))[v];
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

}  // namespace

void kmeans_plan(int N, int k, int* chunk, int* nchunks) {
    int ch = 256;
    while (ch < KM_MAX_CHUNK && ((int64_t)(N + ch - 1) / ch) * k * 4 > ((int64_t)64 << 20)) ch *= 2;
    *chunk = ch;
    *nchunks = N > 0 ? (N + ch - 1) / ch : 1;
}

hipError_t launch_kmeans_argmax_rows(const float* qsim, int64_t ld, int k, int rows, int32_t* label, float* sim, long long* moved,
                                     const int* run_if, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (k < 1 || (ld & 3) != 0 || ld < k || ((uintptr_t)qsim & 15) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmeans_argmax_rows, dim3((rows + 3) / 4), dim3(256), 0, s, qsim, ld, k, rows, label, sim, moved, run_if);
    return hipGetLastError();
}

hipError_t launch_kmeans_update(const uint16_t* emb, const int32_t* label, int N, int d, int k, double* sums, int32_t* counts,
                                uint16_t* centroids, const KmeansScratch& ws, const int* run_if, hipStream_t s) {
    if (N < 1 || k < 1 || d < 64 || (d & 63) != 0 || ws.chunk < 256 || ws.chunk > KM_MAX_CHUNK || (ws.chunk & 255) != 0 ||
        (int64_t)ws.nchunks * ws.chunk < N || (int64_t)(ws.nchunks - 1) * ws.chunk >= N)
        return hipErrorInvalidValue;
    const int64_t ncnt = (int64_t)ws.nchunks * k;
    hipLaunchKernelGGL(km_zero, dim3(ncnt > (int64_t)4096 * 256 ? 4096u : blocks_for(ncnt, 256)), dim3(256), 0, s, ws.cnt, ncnt, run_if);
    hipLaunchKernelGGL(km_rank, dim3(ws.nchunks), dim3(256), (size_t)ws.chunk * sizeof(int), s, label, N, k, ws.chunk, ws.rank, ws.cnt, run_if);
    hipLaunchKernelGGL(km_chunk_scan, dim3(blocks_for(k, 4)), dim3(256), 0, s, ws.cnt, ws.nchunks, k, counts, run_if);
    hipLaunchKernelGGL(km_starts, dim3(1), dim3(1024), 0, s, counts, k, ws.start, run_if);
    hipLaunchKernelGGL(km_scatter, dim3(blocks_for(N, 256)), dim3(256), 0, s, label, N, k, ws.chunk, ws.nchunks, ws.rank, ws.cnt, ws.start, ws.order, run_if);
    hipLaunchKernelGGL(km_sum, dim3((unsigned)((int64_t)k * (d >> 6))), dim3(64), 0, s, emb, N, d, k, ws.order, ws.start, counts, sums, run_if);
    const int lds = d <= 4096;  // the sums row in LDS (32 KiB at the most) for the one lane that walks it
    hipLaunchKernelGGL(km_centroid, dim3(k), dim3(256), lds ? (size_t)d * sizeof(double) : 0, s, sums, counts, d, centroids, lds, run_if);
    return hipGetLastError();
}

hipError_t launch_kmeans_step_end(int* ctrl, long long* moved, const float* sim, int N, const int32_t* counts, int k, long long* info,
                                  double* objective, int first, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_step_end, dim3(1), dim3(1024), 0, s, ctrl, moved, sim, N, counts, k, info, objective, first);
    return hipGetLastError();
}

hipError_t launch_kmeans_fill_labels(int32_t* labels, int N, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(km_fill_labels, dim3(blocks_for(N, 256)), dim3(256), 0, s, labels, N);
    return hipGetLastError();
}

hipError_t launch_kmeans_gather_rows(const uint16_t* src, const int32_t* rows, int k, int d, uint16_t* dst, hipStream_t s) {
    if (k <= 0) return hipSuccess;
    if ((d & 7) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(km_gather_rows, dim3(blocks_for((int64_t)k * (d >> 3), 256)), dim3(256), 0, s, src, rows, k, d, dst);
    return hipGetLastError();
}
