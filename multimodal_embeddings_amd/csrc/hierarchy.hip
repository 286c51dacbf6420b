// K19: the cluster hierarchy of the rows of the vector table -- the maximal spanning forest of the mutual-reachability graph
//   m(i, j) = min(core[i], core[j], s(i, j)),  core[i] = the (min_samples - 1)-th largest admissible cosine of row i,
// under the strict total order on edges "m descending, then lo = min(i, j) ascending, then hi = max(i, j) ascending".  The
// order is strict, so the forest is unique (Kruskal's over the same f32 values) and nothing here depends on scheduling.
//
// The cosine blocks are K14's (the MFMA GEMM, EPI_F32), but rows [r0, r0 + m) against ALL columns [0, N): every row sees all
// its partners, so neither kernel needs a reduction per column.  Row i reads s(i, j) and row j reads s(j, i): the same bits,
// because the GEMM accumulates the same products in the same order for both (tests/test_gpu_hierarchy.py holds it to that).
//   hier_core    one workgroup per row: a radix select of the k-th largest value on the order-preserving image of the f32
//                (the high word of best_key), four 8-bit passes with a 256-bin histogram in LDS.  Exact for every k, integer
//                adds only.  A wave whose candidates of one step all fall into one bin (the first pass: cosines share their
//                exponent) adds them with one atomic.
//   hier_scan    one Boruvka round's streaming pass, den_stream's skeleton: one wave per 1024 values of a row, the four 16-byte
//                loads of the cosines, of comp[j] and of core[j] issued before the first test.  A lane keeps the maximum of
//                best_key(min(core[i], core[j], s), j) over its admissible elements of another component; the wave reduces
//                it with shuffles and one lane issues one 64-bit atomicMax on row_key[i].  For a fixed i, "m descending, j
//                ascending" is the edge order restricted to i's pairs, so the row key loses nothing.  The minimum is taken on
//                the ordered images, which is symmetric in i and j whatever the signs of zeros are.
//   hier_merge   O(N) per round: the largest ordered weight per component (32-bit atomicMax), the smallest lo << 32 | hi among
//                the rows that attain it (64-bit atomicMin), then one thread per component root emits the edge unless the
//                component at the other end chose the same edge and has the smaller id, and unites (union_find.h); at last
//                comp is flattened to canonical roots, the keys are cleared and the counters updated.
// A component's chosen edge is its maximal outgoing edge in a strict total order, so the chosen edges never close a cycle and
// at least half of the components with an outgoing edge disappear per round: at most ceil(log2 N) rounds emit edges.
#include "common.h"
#include "hierarchy.h"
#include "union_find.h"

namespace {

constexpr int SEG = 1024;  // values of one row a wave of hier_scan handles: 4 steps of 64 lanes x 4

__device__ __forceinline__ uint32_t ordered(float s) { return (uint32_t)(best_key(s, 0) >> 32); }
__device__ __forceinline__ float unordered(uint32_t o) { return key_sim((unsigned long long)o << 32); }

__global__ __launch_bounds__(256) void hier_init(HierState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        st.parent[i] = i;
        st.row_key[i] = 0ull;
        st.comp_weight[i] = 0u;
        st.comp_edge[i] = ~0ull;
    }
    if (i < ((N + 3) & ~3)) {  // the padding rows belong to no component
        st.comp[i] = i < N ? i : -1;
        st.core[i] = 0.f;
    }
    if (i < 3) st.counters[i] = i == 2 ? (unsigned long long)N : 0ull;
}

__global__ __launch_bounds__(256) void hier_fill_core(float* __restrict__ core, int r0, int m, float value) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < m) core[r0 + a] = value;
}

// one workgroup per row
__global__ __launch_bounds__(256) void hier_core(const float* __restrict__ block, int64_t ld, int N, int r0, const int32_t* __restrict__ group,
                                                 uint32_t k, float* __restrict__ core) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t pick[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = r0 + (int)blockIdx.x;
    const float* src = block + (int64_t)blockIdx.x * ld;
    const int gi = group ? group[i] : 0;
    uint32_t prefix = 0, mask = 0, kk = k;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        if (tid == 0) pick[0] = 0xffffffffu;
        __syncthreads();
        // rows start 16-byte aligned and ld >= N rounded up to 4: a load that starts below N stays inside the row
        for (int b0 = 0; b0 < N; b0 += 1024) {
            const int b = b0 + 4 * tid;
            const float4 v = b < N ? *(const float4*)(src + b) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int j = b + t;
                bool ok = j < N && j != i;
                if (ok && group) ok = group[j] != gi;
                const uint32_t o = ordered(e[t]);
                ok = ok && (o & mask) == prefix;
                const uint32_t bin = (o >> shift) & 255u;
                const uint64_t act = __ballot(ok);
                if (act == 0) continue;
                const int leader = __builtin_ctzll(act);
                const uint32_t first = __shfl(bin, leader);
                if (__ballot(ok && bin == first) == act) {
                    if (lane == leader) atomicAdd(&hist[first], (uint32_t)__popcll(act));
                } else if (ok) {
                    atomicAdd(&hist[bin], 1u);
                }
            }
        }
        __syncthreads();
        // suf = the candidates in the bins tid..255; the digit is the one bin with suf >= kk > suf - h
        const uint32_t h = hist[tid];
        uint32_t suf = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_down(suf, o);
            if (lane + o < 64) suf += up;
        }
        if (lane == 0) wsum[wave] = suf;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) suf += wsum[w];
        if (suf >= kk && suf - h < kk) {
            pick[0] = (uint32_t)tid;
            pick[1] = kk - (suf - h);
        }
        __syncthreads();
        const uint32_t digit = pick[0];
        if (digit == 0xffffffffu) {  // fewer than k admissible partners (the first pass only): below every cosine
            if (tid == 0) core[i] = -2.0f;
            return;
        }
        kk = pick[1];
        prefix |= digit << shift;
        mask |= 0xffu << shift;
        __syncthreads();  // pick is read before the next pass resets it
    }
    if (tid == 0) core[i] = unordered(prefix);
}

__global__ __launch_bounds__(256) void hier_scan(const float* __restrict__ block, int64_t ld, int m, int N, int r0,
                                                 const int32_t* __restrict__ group, HierState st, int segs) {
    const int lane = threadIdx.x & 63;
    const int rb = blockIdx.x / segs, seg = blockIdx.x - rb * segs;
    const int a = rb * 4 + (threadIdx.x >> 6);
    if (a >= m) return;  // whole wave
    const int i = r0 + a;
    const int b0 = seg * SEG;
    if (b0 >= N) return;
    const float* src = block + (int64_t)a * ld;

    // comp and core hold N rounded up to 4 entries, 16-byte aligned, as the rows of the block: a load that starts below N stays inside
    float4 v[4], kc[4];
    int4 cc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = b0 + q * 256 + 4 * lane;
        const bool in = b < N;
        v[q] = in ? *(const float4*)(src + b) : make_float4(0.f, 0.f, 0.f, 0.f);
        kc[q] = in ? *(const float4*)(st.core + b) : make_float4(0.f, 0.f, 0.f, 0.f);
        cc[q] = in ? *(const int4*)(st.comp + b) : make_int4(-1, -1, -1, -1);
    }
    const float e[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                         v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
    const float kj[16] = {kc[0].x, kc[0].y, kc[0].z, kc[0].w, kc[1].x, kc[1].y, kc[1].z, kc[1].w,
                          kc[2].x, kc[2].y, kc[2].z, kc[2].w, kc[3].x, kc[3].y, kc[3].z, kc[3].w};
    const int cj[16] = {cc[0].x, cc[0].y, cc[0].z, cc[0].w, cc[1].x, cc[1].y, cc[1].z, cc[1].w,
                        cc[2].x, cc[2].y, cc[2].z, cc[2].w, cc[3].x, cc[3].y, cc[3].z, cc[3].w};
    const int ci = st.comp[i];
    const uint32_t oi = ordered(st.core[i]);
    const int gi = group ? group[i] : 0;
    unsigned long long best = 0ull;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int j = b0 + (t >> 2) * 256 + 4 * lane + (t & 3);
        bool ok = j < N && cj[t] != ci;  // j == i has comp[j] == comp[i]
        if (ok && group) ok = group[j] != gi;
        const uint32_t o = min(oi, min(ordered(kj[t]), ordered(e[t])));
        const unsigned long long key = ((unsigned long long)o << 32) | (0xffffffffu - (uint32_t)j);
        if (ok && key > best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if (lane == 0 && best != 0ull) (void)__hip_atomic_fetch_max(st.row_key + i, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the largest ordered weight among the keys of a component's rows
__global__ __launch_bounds__(256) void hier_select_weight(HierState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long key = st.row_key[i];
    if (key) (void)__hip_atomic_fetch_max(st.comp_weight + st.comp[i], (uint32_t)(key >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// among the rows that attain it, the smallest (lo, hi)
__global__ __launch_bounds__(256) void hier_select_edge(HierState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long key = st.row_key[i];
    if (!key) return;
    const int c = st.comp[i];
    if ((uint32_t)(key >> 32) != st.comp_weight[c]) return;
    const uint32_t j = 0xffffffffu - (uint32_t)key;
    const uint32_t lo = min((uint32_t)i, j), hi = max((uint32_t)i, j);
    (void)__hip_atomic_fetch_min(st.comp_edge + c, ((unsigned long long)lo << 32) | hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per component root: emit and unite
__global__ __launch_bounds__(256) void hier_merge(HierState st, int N) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N || st.comp[c] != c) return;
    const unsigned long long edge = st.comp_edge[c];
    if (edge == ~0ull) return;
    const int lo = (int)(edge >> 32), hi = (int)(uint32_t)edge;
    if (lo < 0 || hi >= N || lo >= hi) return;  // cannot happen: the keys hold rows of the table
    const int clo = st.comp[lo], other = clo == c ? st.comp[hi] : clo;
    if (other < c && st.comp_edge[other] == edge) return;  // both ends chose this edge: the smaller id emits it
    const unsigned long long slot = __hip_atomic_fetch_add(st.counters, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot < (unsigned long long)(N - 1)) {  // a forest has at most N - 1 edges
        st.edges[2 * slot] = lo;
        st.edges[2 * slot + 1] = hi;
        st.weights[slot] = unordered(st.comp_weight[c]);
    }
    unite(st.parent, lo, hi);
}

// nothing else runs on the state now: a read-only walk
__device__ __forceinline__ int root_of(const int32_t* parent, int x) {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}

__global__ __launch_bounds__(256) void hier_flatten(HierState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        st.comp[i] = root_of(st.parent, i);
        st.row_key[i] = 0ull;
        st.comp_weight[i] = 0u;
        st.comp_edge[i] = ~0ull;
    }
    if (i == 0) {
        st.counters[1] += 1ull;
        st.counters[2] = (unsigned long long)N - st.counters[0];
    }
}

bool block_ok(const float* block, int64_t ld, int N, const HierState& st) {
    return (ld & 3) == 0 && ld >= N && ((uintptr_t)block & 15) == 0 && ((uintptr_t)st.core & 15) == 0 && ((uintptr_t)st.comp & 15) == 0;
}

unsigned blocks_of(int n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

}  // namespace

hipError_t launch_hier_init(const HierState& st, int N, hipStream_t s) {
    hipLaunchKernelGGL(hier_init, dim3(blocks_of((N + 3) & ~3)), dim3(256), 0, s, st, N);
    return hipGetLastError();
}

hipError_t launch_hier_fill_core(const HierState& st, int r0, int m, float value, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(hier_fill_core, dim3(blocks_of(m)), dim3(256), 0, s, st.core, r0, m, value);
    return hipGetLastError();
}

hipError_t launch_hier_core(const float* block, int64_t ld, int m, int N, int r0, const int32_t* group, int k, const HierState& st, hipStream_t s) {
    if (m <= 0 || N <= 0) return hipSuccess;
    if (k < 1 || !block_ok(block, ld, N, st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hier_core, dim3((unsigned)m), dim3(256), 0, s, block, ld, N, r0, group, (uint32_t)k, st.core);
    return hipGetLastError();
}

hipError_t launch_hier_scan(const float* block, int64_t ld, int m, int N, int r0, const int32_t* group, const HierState& st, hipStream_t s) {
    if (m <= 0 || N <= 0) return hipSuccess;
    if (!block_ok(block, ld, N, st)) return hipErrorInvalidValue;
    const int segs = (N + SEG - 1) / SEG;
    const int64_t b = (int64_t)((m + 3) / 4) * segs;
    if (b > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hier_scan, dim3((unsigned)b), dim3(256), 0, s, block, ld, m, N, r0, group, st, segs);
    return hipGetLastError();
}

hipError_t launch_hier_merge(const HierState& st, int N, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    const unsigned blocks = blocks_of(N);
    hipLaunchKernelGGL(hier_select_weight, dim3(blocks), dim3(256), 0, s, st, N);
    hipLaunchKernelGGL(hier_select_edge, dim3(blocks), dim3(256), 0, s, st, N);
    hipLaunchKernelGGL(hier_merge, dim3(blocks), dim3(256), 0, s, st, N);
    hipLaunchKernelGGL(hier_flatten, dim3(blocks), dim3(256), 0, s, st, N);
    return hipGetLastError();
}
