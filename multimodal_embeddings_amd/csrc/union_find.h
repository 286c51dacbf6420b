// The device pieces K14 (duplicates.hip) and K18 (density.hip) share: the lock-free union-find with canonical roots, the
// packed best-partner key, and the relaxed agent-scope add.  duplicates.hip's head explains the scheme.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ int ld_parent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_parent(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_root(int32_t* parent, int x) {
    for (;;) {
        const int p = ld_parent(parent + x);
        if (p == x) return x;
        const int gp = ld_parent(parent + p);
        if (gp == p) return p;
        st_parent(parent + x, gp);  // x is not a root and never becomes one again; gp is an ancestor of x
        x = gp;
    }
}

__device__ __forceinline__ void unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;  // in a dense group almost every edge ends here
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = hi;  // hooked by someone else meanwhile: walk on from its new parent
        b = lo;
    }
}

// order-preserving image of an f32 in the high word, 0xffffffff - partner in the low word: the maximum of the keys is the
// most similar partner, the lower index among bit-equal values.  0 is no key (its high word would be a NaN's).
__device__ __forceinline__ unsigned long long best_key(float s, int partner) {
    const uint32_t u = __float_as_uint(s);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (0xffffffffu - (uint32_t)partner);
}
__device__ __forceinline__ float key_sim(unsigned long long k) {
    const uint32_t o = (uint32_t)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <class T>
__device__ __forceinline__ void add_relaxed(T* p, T v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace
