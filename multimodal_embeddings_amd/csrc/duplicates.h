// K14 near-duplicate groups (duplicates.hip): launcher declarations shared with capi_duplicates.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The device side of mme_dup_state (include/mme.h), same fields.
struct DupState {
    int32_t* parent;             // [N] union-find forest, parent[i] <= i
    int32_t* degree;             // [N]
    unsigned long long* best;    // [N] packed (ordered f32 bits << 32) | (0xffffffff - partner); 0 = none
    int32_t* page_pairs;         // [P, P] or null
    int32_t* edges;              // [edge_cap, 2] or null
    float* edge_sim;             // [edge_cap] or null
    unsigned long long* counters;  // [2]: edges found, edges written
    int64_t edge_cap;
    int P;
};

// parent[i] = i, everything else zero
hipError_t launch_dup_init(const DupState& st, int N, hipStream_t s);
// block f32 [m, ld] (ld % 4 == 0, 16-byte aligned): block[a][b] = cosine of rows (r0 + a, c0 + b), b < cols.  Every pair
// with c0 + b > r0 + a, value >= min_sim and group[i] != group[j] (group may be null) is recorded in `st`.
hipError_t launch_dup_scan(const float* block, int64_t ld, int m, int cols, int r0, int c0, const int32_t* group, const int32_t* page_of,
                           float min_sim, const DupState& st, hipStream_t s);
// dst <- dst merged with src (states over the same N rows); edge lists are not merged
hipError_t launch_dup_merge(const DupState& dst, const DupState& src, int N, hipStream_t s);
// labels[i] = smallest row of i's component, best unpacked, summary int64[4] = {edges, groups of >= 2 rows, rows in such
// groups, rows of the largest such group (0 when there is none)}; hist: int32 [N] scratch
hipError_t launch_dup_finish(const DupState& st, int N, int32_t* labels, int32_t* best_idx, float* best_sim, long long* summary, int32_t* hist,
                             hipStream_t s);
