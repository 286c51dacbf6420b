// K17 centring, reduction and whitening of the vector table (projection.hip): launcher declarations shared with
// capi_projection.hip.  The definitions are in include/mme.h (K17) and DESIGN.md 4.27.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mme.h"

constexpr int PJ_TILE = 64;  // columns of one tile of the second-moment matrix; d % 64 == 0
// upper-triangle tile pairs (ta <= tc) of a d x d matrix, and the f64 values one row block leaves per launch
inline int moments_pairs(int d) { const int T = d / PJ_TILE; return T * (T + 1) / 2; }
inline size_t moments_block_values(int d) { return (size_t)moments_pairs(d) * PJ_TILE * PJ_TILE + (size_t)d; }

// K17a, the blocks b0 .. b0 + nb - 1 of MME_MOMENTS_BLOCK rows of emb bf16 [N, d] (16-byte aligned, d % 64 == 0, d <= 1024):
// part f64 [nb][pairs][64][64] = the tiles P_b[ta, tc] of the upper triangle, psum f64 [nb][d] = p_b; every sum from +0.0 in
// ascending row order, one lane per element.  nb <= 65535.
hipError_t launch_moments_block(const uint16_t* emb, int64_t N, int d, int64_t b0, int nb, double* part, double* psum, hipStream_t s);
// sum[c] and gram[a, c] (f64 [d], [d, d]) = (first ? +0.0 : what they hold) + the nb partials in ascending block order;
// the lower triangle of gram is written as the mirror of the upper one.
hipError_t launch_moments_reduce(const double* part, const double* psum, int nb, int d, int first, double* sum, double* gram, hipStream_t s);
// K17b: y[i, j] = sum_c (f32(x[i, c]) - mean[c]) * w[j, c] in f32, i < rows, j < m, into y0 (pitch ld0) and / or y1 (pitch ld1);
// columns m .. ld - 1 are not written.  emb, mean, w, y0, y1 16-byte aligned, d % 64 == 0, ld % 4 == 0.
hipError_t launch_project_rows(const uint16_t* emb, int64_t rows, int d, const float* mean, const float* w, int m, float* y0, int64_t ld0,
                               float* y1, int64_t ld1, hipStream_t s);
