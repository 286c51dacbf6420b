// K18 density clusters (density.hip): launcher declarations shared with capi_density.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The device side of mme_density_state (include/mme.h), same fields.
struct DenState {
    int32_t* count;                // [N] neighbours of the row, self not counted
    int32_t* parent;               // [N] union-find forest over the core rows, parent[i] <= i
    unsigned long long* border;    // [N] best core neighbour of a non-core row as a packed key (union_find.h); 0 = none
    unsigned long long* counters;  // [2]: neighbour pairs the count pass found, neighbour pairs the link pass saw
};

// parent[i] = i, everything else zero
hipError_t launch_den_init(const DenState& st, int N, hipStream_t s);
// block f32 [m, ld] (ld % 4 == 0, 16-byte aligned): block[a][b] = cosine of rows (r0 + a, c0 + b), b < cols.  A neighbour pair
// is one with c0 + b > r0 + a, value >= min_sim and group[i] != group[j] (group may be null).
// count: every pair adds 1 to count[i], count[j] and counters[0].
hipError_t launch_den_count(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, float min_sim,
                            const DenState& st, hipStream_t s);
// link: `count` is final.  A pair of two core rows (count + 1 >= min_samples) is united, a pair of one core row offers it to
// the other row's border key; every pair adds 1 to counters[1].
hipError_t launch_den_link(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, float min_sim,
                           int min_samples, const DenState& st, hipStream_t s);
// labels / kind / border_idx / border_sim per row, summary int64[6] = {pairs, clusters, core, border, noise rows, rows of the
// largest cluster}; hist: int32 [N] scratch
hipError_t launch_den_finish(const DenState& st, int N, int min_samples, int32_t* labels, int32_t* kind, int32_t* border_idx,
                             float* border_sim, long long* summary, int32_t* hist, hipStream_t s);
