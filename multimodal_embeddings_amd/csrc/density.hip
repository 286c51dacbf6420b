// K18: density clusters (DBSCAN) of the rows of the vector table -- the connected components of the CORE rows of the graph
// "cosine >= min_sim between rows of different groups", a core row being one with at least min_samples - 1 neighbours; a
// non-core row next to a core row is a border member of its most similar core neighbour's cluster, every other row is noise.
//
// Whether a row is core is known only when every pair has been counted, so the cosine blocks (K14's: the MFMA GEMM, EPI_F32,
// rows [r0, r0 + m) against columns [c0, N)) are streamed twice, by two kernels that share one skeleton, `den_stream` --
// dup_scan's: one wave reads 1024 consecutive values of one row (four 16-byte loads per lane, all issued before the first
// test) and tests `j > i && s >= min_sim`; a ballot sends the wave on unless some lane found a candidate.  What is done per
// round of up to 64 neighbour pairs (i, j) is the template argument:
//   den_count  count[i] += the round's pairs (one add of the wave), count[j] += 1 per lane (64 consecutive words at most),
//              counters[0] += the round's pairs;
//   den_link   reads count[i] (once per wave) and count[j]: two core rows are united (union_find.h: the root of a component
//              is its smallest member whatever the interleaving was), one core row is offered to the other row's border key
//              with an atomicMax, so the key that stays is the most similar core neighbour, the lower index among bit-equal
//              values, whatever the order of arrival; counters[1] += the round's pairs.
// Both passes read the same f32 values from the same GEMM on the same operands and apply the same test, so they see the same
// pairs: after passes that cover every row counters[0] == counters[1].  Integer adds, maxima of packed keys and the canonical
// union-find only: every output is bit-identical from run to run.  `count` is written by den_count's atomics and read by
// den_link with plain loads: a kernel boundary on one stream lies between them.
#include "common.h"
#include "density.h"
#include "union_find.h"

namespace {

constexpr int SEG = 1024;  // values of one row a wave handles: 4 steps of 64 lanes x 4

__global__ __launch_bounds__(256) void den_init(DenState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        st.parent[i] = i;
        st.count[i] = 0;
        st.border[i] = 0ull;
    }
    if (i < 2) st.counters[i] = 0ull;
}

// op.begin(i): once per wave that has a candidate; op.round(i, j, s, act, bm, lane): the lanes with `act` hold a neighbour
// pair (i, j) of cosine s, bm = __ballot(act) != 0
template <class Op>
__device__ __forceinline__ void den_stream(const float* __restrict__ block, int64_t ld, int m, int cols, int r0, int c0,
                                           const int32_t* __restrict__ group, float min_sim, int segs, Op op) {
    const int lane = threadIdx.x & 63;
    const int rb = blockIdx.x / segs, seg = blockIdx.x - rb * segs;
    const int a = rb * 4 + (threadIdx.x >> 6);
    if (a >= m) return;  // whole wave
    const int i = r0 + a;
    const int first = i - c0 + 1;  // first column of the block with j > i
    const int b0 = seg * SEG;
    if (b0 >= cols || min(b0 + SEG, cols) <= first) return;  // left of the diagonal
    const float* src = block + (int64_t)a * ld;

    // rows start 16-byte aligned and ld >= cols rounded up to 4: a load that starts below `cols` stays inside the row
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = b0 + q * 256 + 4 * lane;
        v[q] = b < cols ? *(const float4*)(src + b) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float e[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                         v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
    uint32_t mask = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int b = b0 + (t >> 2) * 256 + 4 * lane + (t & 3);
        if (b < cols && b >= first && e[t] >= min_sim) mask |= 1u << t;
    }
    if (__ballot(mask != 0) == 0) return;  // the fast path: nothing in these 1024 values

    const int gi = group ? group[i] : 0;
    op.begin(i);
    while (__ballot(mask != 0) != 0) {  // one candidate per lane and round
        bool act = mask != 0;
        const int t = act ? __ffs(mask) - 1 : 0;
        mask &= mask - 1;
        float s = e[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) s = t == k ? e[k] : s;
        const int j = c0 + b0 + (t >> 2) * 256 + 4 * lane + (t & 3);
        if (act && group) act = group[j] != gi;
        const uint64_t bm = __ballot(act);
        if (bm == 0) continue;
        op.round(i, j, s, act, bm, lane);
    }
}

struct CountOp {
    DenState st;
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ void round(int i, int j, float, bool act, uint64_t bm, int lane) {
        if (lane == __builtin_ctzll(bm)) {  // one pair-counter and one count[i] update per wave
            const int n = __popcll(bm);
            add_relaxed(st.counters, (unsigned long long)n);
            add_relaxed(st.count + i, n);
        }
        if (act) add_relaxed(st.count + j, 1);
    }
};

struct LinkOp {
    DenState st;
    int need;  // a row is core when count >= need = min_samples - 1
    bool core_i;
    __device__ __forceinline__ void begin(int i) { core_i = st.count[i] >= need; }
    __device__ __forceinline__ void round(int i, int j, float s, bool act, uint64_t bm, int lane) {
        if (lane == __builtin_ctzll(bm)) add_relaxed(st.counters + 1, (unsigned long long)__popcll(bm));
        if (!act) return;
        const bool core_j = st.count[j] >= need;  // a non-core row i looks for core partners only
        if (core_i && core_j)
            unite(st.parent, i, j);
        else if (core_i)
            (void)__hip_atomic_fetch_max(st.border + j, best_key(s, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (core_j)
            (void)__hip_atomic_fetch_max(st.border + i, best_key(s, j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(256) void den_count(const float* __restrict__ block, int64_t ld, int m, int cols, int r0, int c0,
                                                 const int32_t* __restrict__ group, float min_sim, DenState st, int segs) {
    den_stream(block, ld, m, cols, r0, c0, group, min_sim, segs, CountOp{st});
}

__global__ __launch_bounds__(256) void den_link(const float* __restrict__ block, int64_t ld, int m, int cols, int r0, int c0,
                                                const int32_t* __restrict__ group, float min_sim, int need, DenState st, int segs) {
    den_stream(block, ld, m, cols, r0, c0, group, min_sim, segs, LinkOp{st, need, false});
}

// nothing else runs on the state now: a read-only walk
__device__ __forceinline__ int root_of(const int32_t* parent, int x) {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}

// one thread per row; summary[1..4] by one integer add per wave
__global__ __launch_bounds__(256) void den_finish_rows(DenState st, int N, int need, int32_t* __restrict__ labels, int32_t* __restrict__ kind,
                                                       int32_t* __restrict__ border_idx, float* __restrict__ border_sim,
                                                       int32_t* __restrict__ hist, long long* __restrict__ summary) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool row = i < N;
    int k = 0, lab = -1, bi = -1;
    float bs = 0.f;
    if (row) {
        if (st.count[i] >= need) {
            k = 2;
            lab = root_of(st.parent, i);  // the smallest core row of the component
        } else {
            const unsigned long long key = st.border[i];
            if (key) {
                k = 1;
                bi = (int32_t)(0xffffffffu - (uint32_t)key);
                bs = key_sim(key);
                lab = root_of(st.parent, bi);
            }
        }
        labels[i] = lab;
        kind[i] = k;
        border_idx[i] = bi;
        border_sim[i] = bs;
        if (lab >= 0) add_relaxed(hist + lab, 1);
    }
    const uint64_t roots = __ballot(k == 2 && lab == i), core = __ballot(k == 2), bord = __ballot(k == 1), noise = __ballot(row && k == 0);
    if ((threadIdx.x & 63) == 0) {
        if (roots) add_relaxed(summary + 1, (long long)__popcll(roots));
        if (core) add_relaxed(summary + 2, (long long)__popcll(core));
        if (bord) add_relaxed(summary + 3, (long long)__popcll(bord));
        if (noise) add_relaxed(summary + 4, (long long)__popcll(noise));
    }
}

// integer atomics only: the summary does not depend on the order of arrival
__global__ __launch_bounds__(256) void den_finish_summary(DenState st, int N, const int32_t* __restrict__ hist, long long* __restrict__ summary) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int big = i < N ? hist[i] : 0;
    if (__ballot(big != 0)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) big = max(big, __shfl_xor(big, o));
        if ((threadIdx.x & 63) == 0) (void)__hip_atomic_fetch_max(summary + 5, (long long)big, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (i == 0) summary[0] = (long long)st.counters[0];
}

// the checks of a block, and the grid: one wave per row and 1024 columns
bool block_grid(const float* block, int64_t ld, int cols, int r0, int c0, int m, int* segs, unsigned* blocks) {
    if ((ld & 3) != 0 || ld < cols || c0 > r0 || ((uintptr_t)block & 15) != 0) return false;
    *segs = (cols + SEG - 1) / SEG;
    const int64_t b = (int64_t)((m + 3) / 4) * *segs;
    if (b > 0x7fffffffll) return false;
    *blocks = (unsigned)b;
    return true;
}

}  // namespace

hipError_t launch_den_init(const DenState& st, int N, hipStream_t s) {
    hipLaunchKernelGGL(den_init, dim3((N + 255) / 256 > 0 ? (N + 255) / 256 : 1), dim3(256), 0, s, st, N);
    return hipGetLastError();
}

hipError_t launch_den_count(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, float min_sim,
                            const DenState& st, hipStream_t s) {
    if (m <= 0 || cols <= 0) return hipSuccess;
    int segs;
    unsigned blocks;
    if (!block_grid(block, ld, cols, r0, c0, m, &segs, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(den_count, dim3(blocks), dim3(256), 0, s, block, ld, m, cols, r0, c0, group, min_sim, st, segs);
    return hipGetLastError();
}

hipError_t launch_den_link(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, float min_sim,
                           int min_samples, const DenState& st, hipStream_t s) {
    if (m <= 0 || cols <= 0) return hipSuccess;
    int segs;
    unsigned blocks;
    if (min_samples < 1 || !block_grid(block, ld, cols, r0, c0, m, &segs, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(den_link, dim3(blocks), dim3(256), 0, s, block, ld, m, cols, r0, c0, group, min_sim, min_samples - 1, st, segs);
    return hipGetLastError();
}

hipError_t launch_den_finish(const DenState& st, int N, int min_samples, int32_t* labels, int32_t* kind, int32_t* border_idx,
                             float* border_sim, long long* summary, int32_t* hist, hipStream_t s) {
    if (min_samples < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(summary, 0, 6 * sizeof(long long), s);
    if (e != hipSuccess) return e;
    const int blocks = N > 0 ? (N + 255) / 256 : 1;
    if (N > 0) {
        if ((e = hipMemsetAsync(hist, 0, (size_t)N * sizeof(int32_t), s)) != hipSuccess) return e;
        hipLaunchKernelGGL(den_finish_rows, dim3(blocks), dim3(256), 0, s, st, N, min_samples - 1, labels, kind, border_idx, border_sim, hist, summary);
    }
    hipLaunchKernelGGL(den_finish_summary, dim3(blocks), dim3(256), 0, s, st, N, hist, summary);
    return hipGetLastError();
}
