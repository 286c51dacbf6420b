// K19 cluster hierarchy (hierarchy.hip): launcher declarations shared with capi_hierarchy.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The device side of mme_hierarchy_state (include/mme.h), same fields.
struct HierState {
    float* core;                    // [N rounded up to 4] core similarity of the row
    int32_t* comp;                  // [N rounded up to 4] canonical root (smallest member) of the row's component
    unsigned long long* row_key;    // [N] best outgoing edge of the row in this round as a packed key (union_find.h); 0 = none
    int32_t* parent;                // [N] union-find forest, parent[i] <= i
    uint32_t* comp_weight;          // [N] per component root: the largest ordered weight among its rows' keys
    unsigned long long* comp_edge;  // [N] per component root: lo << 32 | hi of its chosen edge, ~0 = none
    int32_t* edges;                 // [N - 1, 2]
    float* weights;                 // [N - 1]
    unsigned long long* counters;   // [3]: edges emitted, rounds run, components left
};

// parent[i] = comp[i] = i, keys cleared, counters = {0, 0, N}
hipError_t launch_hier_init(const HierState& st, int N, hipStream_t s);
// core[r0 + a] = value, a < m (min_samples = 1: +1.5; a table of one row: -2.0)
hipError_t launch_hier_fill_core(const HierState& st, int r0, int m, float value, hipStream_t s);
// block f32 [m, ld] (ld % 4 == 0, ld >= N, 16-byte aligned): block[a][j] = cosine of rows (r0 + a, j), j < N.
// core[r0 + a] = the k-th largest value of the row over the admissible j (j != i, group[i] != group[j]; group may be null),
// k >= 1; -2.0 when the row has fewer than k admissible partners.
hipError_t launch_hier_core(const float* block, int64_t ld, int m, int N, int r0, const int32_t* group, int k, const HierState& st, hipStream_t s);
// one round's scan of the same rows: row_key[i] = max over the admissible j with comp[j] != comp[i] of
// best_key(min(core[i], core[j], block[a][j]), j)
hipError_t launch_hier_scan(const float* block, int64_t ld, int m, int N, int r0, const int32_t* group, const HierState& st, hipStream_t s);
// the end of a round: every component's maximal edge, the emitted edges, the unions, comp flattened, the keys cleared
hipError_t launch_hier_merge(const HierState& st, int N, hipStream_t s);
