// K14: near-duplicate groups -- the connected components of the graph "cosine >= min_sim between rows of different groups".
//
// The cosine values come from the MFMA GEMM (EPI_F32) as a block [m, ld] of rows [r0, r0 + m) against columns [c0, N);
// `dup_scan` streams that block once.  One wave reads 1024 consecutive values of one row (four 16-byte loads per lane, all
// issued before the first test) and tests `j > i && s >= min_sim`; a ballot sends the wave on unless some lane found a
// candidate, which for a thresholded graph of an archive is the case for a small fraction of the waves.  Only then are the
// group ids read and the edges recorded with agent-scope relaxed atomics: the two degrees, the best partner of both ends
// (atomicMax of a packed key, so the result does not depend on the order of arrival), the page-pair count, the edge list,
// and the union.
//
// Union-find (the lock-free scheme of Jayanti & Tarjan, as ECL-CC uses it): parent[x] <= x always.  `find_root` walks with
// path halving; `unite` takes both roots, and hooks the LARGER root under the smaller one with a compare-and-swap that
// succeeds only while the larger one still is a root.  A failed swap means another edge hooked that root meanwhile: the
// loop starts again from the new parents.  Every hook points a root at a smaller index, path halving replaces a parent by
// an ancestor (also smaller) and never touches a root, so there are no cycles, every walk ends, every successful swap
// removes one root (so the retries are bounded by the number of rows), and when all edges are in, the root of a component
// is its smallest member whatever the interleaving was.  The loads and stores of the walk are single 32-bit accesses (no
// read-modify-write), issued at agent scope so that they are served by the L2 all CUs share: through a CU's own vector
// cache a lane could keep seeing a stale "x is a root" and retry a swap that can no longer succeed.
#include "common.h"
#include "duplicates.h"
#include "union_find.h"

namespace {

constexpr int SEG = 1024;  // values of one row a wave handles: 4 steps of 64 lanes x 4

__global__ __launch_bounds__(256) void dup_init(DupState st, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        st.parent[i] = i;
        st.degree[i] = 0;
        st.best[i] = 0ull;
    }
    if (i < 2) st.counters[i] = 0ull;
}

__global__ __launch_bounds__(256) void dup_scan(const float* __restrict__ block, int64_t ld, int m, int cols, int r0, int c0,
                                                const int32_t* __restrict__ group, const int32_t* __restrict__ page_of, float min_sim,
                                                DupState st, int segs) {
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
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const unsigned long long cap = (unsigned long long)st.edge_cap;
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
        const int n = __popcll(bm), leader = __builtin_ctzll(bm);
        // one slot range and one degree[i] update per wave
        unsigned long long base = 0;
        if (lane == leader) {
            base = __hip_atomic_fetch_add(st.counters, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st.edges && base < cap) add_relaxed(st.counters + 1, cap - base < (unsigned long long)n ? cap - base : (unsigned long long)n);
            add_relaxed(st.degree + i, n);
        }
        const uint32_t blo = __builtin_amdgcn_readlane((uint32_t)base, leader), bhi = __builtin_amdgcn_readlane((uint32_t)(base >> 32), leader);
        base = ((unsigned long long)bhi << 32) | blo;
        if (!act) continue;
        add_relaxed(st.degree + j, 1);
        (void)__hip_atomic_fetch_max(st.best + i, best_key(s, j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(st.best + j, best_key(s, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st.page_pairs) {
            const int p = page_of[i], q = page_of[j];
            if ((unsigned)p < (unsigned)st.P && (unsigned)q < (unsigned)st.P) {
                add_relaxed(st.page_pairs + (int64_t)p * st.P + q, 1);
                if (p != q) add_relaxed(st.page_pairs + (int64_t)q * st.P + p, 1);
            }
        }
        if (st.edges) {
            const unsigned long long slot = base + (unsigned)__popcll(bm & below);
            if (slot < cap) {
                st.edges[2 * slot] = i;
                st.edges[2 * slot + 1] = j;
                st.edge_sim[slot] = s;
            }
        }
        unite(st.parent, i, j);
    }
}

// one thread per row (and per page pair)
__global__ __launch_bounds__(256) void dup_merge(DupState dst, DupState src, int N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        unite(dst.parent, (int)i, src.parent[i]);  // src.parent[i] is in i's component of src: all of them restate src's forest
        dst.degree[i] += src.degree[i];
        const unsigned long long kb = src.best[i];
        if (kb > dst.best[i]) dst.best[i] = kb;
    }
    if (dst.page_pairs && i < (int64_t)dst.P * dst.P) dst.page_pairs[i] += src.page_pairs[i];
    if (i == 0) dst.counters[0] += src.counters[0];  // edges found; dst's list, and the count of what it holds, stay
}

__global__ __launch_bounds__(256) void dup_finish_rows(DupState st, int N, int32_t* __restrict__ labels, int32_t* __restrict__ best_idx,
                                                       float* __restrict__ best_sim, int32_t* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int x = i;  // nothing else runs on the state now: a read-only walk
    for (int p = st.parent[x]; p != x; p = st.parent[x]) x = p;
    labels[i] = x;
    add_relaxed(hist + x, 1);
    const unsigned long long k = st.best[i];
    best_idx[i] = k ? (int32_t)(0xffffffffu - (uint32_t)k) : -1;
    best_sim[i] = k ? key_sim(k) : 0.f;
}

// integer atomics only: the summary does not depend on the order of arrival
__global__ __launch_bounds__(256) void dup_finish_summary(DupState st, int N, const int32_t* __restrict__ hist, long long* __restrict__ summary) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c = i < N ? hist[i] : 0;
    const bool grp = c >= 2;
    const uint64_t bm = __ballot(grp);
    if (bm) {
        int rows = grp ? c : 0, big = rows;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            rows += __shfl_xor(rows, o);
            big = max(big, __shfl_xor(big, o));
        }
        if ((threadIdx.x & 63) == 0) {
            add_relaxed(summary + 1, (long long)__popcll(bm));
            add_relaxed(summary + 2, (long long)rows);
            (void)__hip_atomic_fetch_max(summary + 3, (long long)big, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (i == 0) summary[0] = (long long)st.counters[0];
}

}  // namespace

hipError_t launch_dup_init(const DupState& st, int N, hipStream_t s) {
    if (st.page_pairs) {
        hipError_t e = hipMemsetAsync(st.page_pairs, 0, (size_t)st.P * st.P * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dup_init, dim3((N + 255) / 256 > 0 ? (N + 255) / 256 : 1), dim3(256), 0, s, st, N);
    return hipGetLastError();
}

hipError_t launch_dup_scan(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, const int32_t* page_of,
                           float min_sim, const DupState& st, hipStream_t s) {
    if (m <= 0 || cols <= 0) return hipSuccess;
    if ((ld & 3) != 0 || ld < cols || c0 > r0 || ((uintptr_t)block & 15) != 0) return hipErrorInvalidValue;
    const int segs = (cols + SEG - 1) / SEG;
    const int64_t blocks = (int64_t)((m + 3) / 4) * segs;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dup_scan, dim3((unsigned)blocks), dim3(256), 0, s, block, ld, m, cols, r0, c0, group, page_of, min_sim, st, segs);
    return hipGetLastError();
}

hipError_t launch_dup_merge(const DupState& dst, const DupState& src, int N, hipStream_t s) {
    int64_t n = N;
    if (dst.page_pairs && (int64_t)dst.P * dst.P > n) n = (int64_t)dst.P * dst.P;
    if (n <= 0) n = 1;
    hipLaunchKernelGGL(dup_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, N);
    return hipGetLastError();
}

hipError_t launch_dup_finish(const DupState& st, int N, int32_t* labels, int32_t* best_idx, float* best_sim, long long* summary, int32_t* hist,
                             hipStream_t s) {
    hipError_t e = hipMemsetAsync(summary, 0, 4 * sizeof(long long), s);
    if (e != hipSuccess) return e;
    const int blocks = N > 0 ? (N + 255) / 256 : 1;
    if (N > 0) {
        if ((e = hipMemsetAsync(hist, 0, (size_t)N * sizeof(int32_t), s)) != hipSuccess) return e;
        hipLaunchKernelGGL(dup_finish_rows, dim3(blocks), dim3(256), 0, s, st, N, labels, best_idx, best_sim, hist);
    }
    hipLaunchKernelGGL(dup_finish_summary, dim3(blocks), dim3(256), 0, s, st, N, hist, summary);
    return hipGetLastError();
}
