// K15 spherical k-means over the vector table (kmeans.hip): launcher declarations shared with capi_kmeans.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Scratch of one update for N rows and k clusters, carved by the caller (kmeans_plan sizes it).  Rows are handled in
// chunks of `chunk` consecutive rows (a multiple of 256, at most KM_MAX_CHUNK); cnt is [k, nchunks].
constexpr int KM_MAX_CHUNK = 8192;  // its labels sit in LDS: 32 KiB
struct KmeansScratch {
    int32_t* rank;   // [N]  rows of the same cluster before this row inside its chunk
    int32_t* order;  // [N]  the rows sorted by (cluster, row)
    int32_t* start;  // [k]  first position of cluster j in `order`
    int32_t* cnt;    // [k, nchunks]  rows of cluster j in a chunk, then in the chunks before it
    int chunk, nchunks;
};
// chunk and nchunks for (N, k): 256-row chunks while the [k, nchunks] table stays below 64 MiB, larger ones after that
void kmeans_plan(int N, int k, int* chunk, int* nchunks);

// label[row] = the column of the largest of qsim[row, 0..k) (block f32 [rows, ld], ld % 4 == 0, 16-byte aligned), sim[row]
// = that value.  The order is total: a NaN is below every number, -0.0 below +0.0, and among bit-equal values the lowest
// column wins (a row of NaNs: label 0, sim NaN).  *moved += the rows whose label differs from the label[row] found.
hipError_t launch_kmeans_argmax_rows(const float* qsim, int64_t ld, int k, int rows, int32_t* label, float* sim, long long* moved,
                                     const int* run_if, hipStream_t s);
// sums f64 [k, d] = the bf16 rows of emb [N, d] with label == j added up in ascending row order, counts[j] their number;
// centroid[j, :] = bf16(sums[j, :] / max(||sums[j, :]||, 1e-12)) in f64 for the clusters with members, untouched for the
// others.  d % 64 == 0.  A label outside 0..k-1 belongs to no cluster.  No floating-point atomics: bit-identical run to run.
hipError_t launch_kmeans_update(const uint16_t* emb, const int32_t* label, int N, int d, int k, double* sums, int32_t* counts,
                                uint16_t* centroids, const KmeansScratch& ws, const int* run_if, hipStream_t s);
// ctrl: int[2] = {go, unused}; moved: the counter of launch_kmeans_argmax_rows; info int64[4], objective f64[1] as
// mme_kmeans_state.  first != 0 (after the assignment against the start): go = 1, info = 0, objective, moved = 0.
// Otherwise, only while go != 0: iterations += 1, info[1] = moved, go = converged' = (moved != 0), moved = 0, info[3] =
// clusters with counts[j] == 0, objective = the f64 sum of sim[0..N) in a fixed order.
hipError_t launch_kmeans_step_end(int* ctrl, long long* moved, const float* sim, int N, const int32_t* counts, int k, long long* info,
                                  double* objective, int first, hipStream_t s);
// labels[0..N) = -1
hipError_t launch_kmeans_fill_labels(int32_t* labels, int N, hipStream_t s);
// dst[j, :] = src[rows[j], :], bf16 rows of d (d % 8 == 0), j < k
hipError_t launch_kmeans_gather_rows(const uint16_t* src, const int32_t* rows, int k, int d, uint16_t* dst, hipStream_t s);

// K16, the silhouette of a partition (silhouette.hip).  sample[i] (f64 [N]) from the bf16 rows, their labels (outside 0..k-1:
// NaN), and sums / counts as launch_kmeans_update leaves them; d % 64 == 0, emb and sums 16-byte aligned.
hipError_t launch_silhouette_rows(const uint16_t* emb, int N, int d, const int32_t* label, int k, const double* sums, const int32_t* counts,
                                  double* sample, hipStream_t s);
// csum[j] = the samples of cluster j added in a fixed order over order[start[j] .. + counts[j]), cluster[j] = csum[j] / counts[j]
// (NaN for an empty one); info = {rows counted, clusters with members}; score = the sum of csum over those rows, NaN with
// fewer than two clusters with members.
hipError_t launch_silhouette_reduce(const double* sample, const int32_t* order, const int32_t* start, const int32_t* counts, int k, double* csum,
                                    double* cluster, double* score, long long* info, hipStream_t s);
