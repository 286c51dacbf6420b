// C ABI of K17 (include/mme.h, mme_moments / mme_project): argument checks and the host pass.  The moments go through the K12
// workspace as per-block partials, in groups of blocks when all of them do not fit (the groups are added in ascending order on
// top of each other, so the grouping never changes a bit); the projection writes f32 rows and hands them to the existing
// row kernel for the L2 step, through the workspace in row chunks when the caller's f32 rows are not there or not dense.
#include <cstdlib>

#include "ctx.h"
#include "projection.h"

namespace {

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

size_t workspace_cap() {
    static const int64_t ws_mb = getenv("MME_NEIGH_WS_MB") ? atoll(getenv("MME_NEIGH_WS_MB")) : 2048;
    return (size_t)(ws_mb < 1 ? 1 : ws_mb) << 20;
}

int check_moments(mme_ctx* c, const char* who, const uint16_t* emb, int64_t N, int d, const double* sum, const double* gram) {
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(c, MME_E_ARG, "%s: N = %lld; supported 1..2^24", who, (long long)N);
    if (d < 64 || d > 1024 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; supported: a multiple of 64 in 64..1024", who, d);
    if (!emb || !aligned_to(emb, 16)) return fail(c, MME_E_ARG, "%s: emb = %p; a non-null, 16-byte aligned pointer is required", who, (const void*)emb);
    if (!sum || !aligned_to(sum, 8)) return fail(c, MME_E_ARG, "%s: sum = %p; a non-null, 8-byte aligned pointer is required", who, (const void*)sum);
    if (!gram || !aligned_to(gram, 8)) return fail(c, MME_E_ARG, "%s: gram = %p; a non-null, 8-byte aligned pointer is required", who, (const void*)gram);
    return MME_OK;
}

// group_blocks: 0 = as many blocks per group as the workspace holds
int moments(mme_ctx* c, const uint16_t* emb, int64_t N, int d, int group_blocks, double* sum, double* gram, hipStream_t s) {
    const int64_t blocks = (N + MME_MOMENTS_BLOCK - 1) / MME_MOMENTS_BLOCK;
    const size_t per = moments_block_values(d) * sizeof(double);
    int64_t group = group_blocks > 0 ? group_blocks : (int64_t)(workspace_cap() / per);
    if (group < 1) group = 1;
    if (group > 65535) group = 65535;  // the grid's second dimension
    if (group > blocks) group = blocks;
    int r;
    if ((r = ensure(c, c->neigh_ws, (size_t)group * per))) return r;
    double* part = (double*)c->neigh_ws.p;
    double* psum = part + (size_t)group * moments_pairs(d) * PJ_TILE * PJ_TILE;
    Timed t(c, s, KC_CLUSTER);
    for (int64_t b0 = 0; b0 < blocks; b0 += group) {
        const int nb = (int)(blocks - b0 < group ? blocks - b0 : group);
        HIP_TRY(c, launch_moments_block(emb, N, d, b0, nb, part, psum, s));
        HIP_TRY(c, launch_moments_reduce(part, psum, nb, d, b0 == 0, sum, gram, s));
    }
    return MME_OK;
}

}  // namespace

int mme_moments(mme_ctx* c, const uint16_t* emb, int64_t N, int d, double* sum, double* gram, void* stream) {
    if (!c) return MME_E_ARG;
    int r;
    if ((r = check_moments(c, "mme_moments", emb, N, d, sum, gram))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    return moments(c, emb, N, d, 0, sum, gram, (hipStream_t)stream);
}

int mme_moments_apply(mme_ctx* c, const uint16_t* emb, int64_t N, int d, int group_blocks, double* sum, double* gram, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_moments_apply";
    int r;
    if ((r = check_moments(c, who, emb, N, d, sum, gram))) return r;
    if (group_blocks < 0 || group_blocks > 65535) return fail(c, MME_E_ARG, "%s: group_blocks = %d; supported 0..65535", who, group_blocks);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if ((r = moments(c, emb, N, d, group_blocks, sum, gram, s))) return r;
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

int mme_project(mme_ctx* c, const uint16_t* emb, int64_t N, int d, const float* mean, const float* w, int m, float* y_f32, int64_t ld_y,
                uint16_t* y_bf16, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_project";
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(c, MME_E_ARG, "%s: N = %lld; supported 1..2^24", who, (long long)N);
    if (d < 64 || d > 65536 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; supported: a multiple of 64 in 64..65536", who, d);
    if (m < 1 || m > d) return fail(c, MME_E_ARG, "%s: m = %d; supported 1..d (d = %d)", who, m, d);
    if (!y_f32 && !y_bf16) return fail(c, MME_E_ARG, "%s: y_f32 and y_bf16 are both null; at least one output is required", who);
    if (y_bf16 && (m % 64) != 0) return fail(c, MME_E_ARG, "%s: m = %d with y_bf16; supported: m %% 64 == 0 (normalised rows feed K9..K16)", who, m);
    if (y_f32 && (ld_y < m || (ld_y % 4) != 0))
        return fail(c, MME_E_ARG, "%s: ld_y = %lld; supported: a multiple of 4 that is at least m (m = %d)", who, (long long)ld_y, m);
    if (!emb || !aligned_to(emb, 16)) return fail(c, MME_E_ARG, "%s: emb = %p; a non-null, 16-byte aligned pointer is required", who, (const void*)emb);
    if (!mean || !aligned_to(mean, 16)) return fail(c, MME_E_ARG, "%s: mean = %p; a non-null, 16-byte aligned pointer is required", who, (const void*)mean);
    if (!w || !aligned_to(w, 16)) return fail(c, MME_E_ARG, "%s: w = %p; a non-null, 16-byte aligned pointer is required", who, (const void*)w);
    if (!aligned_to(y_f32, 16)) return fail(c, MME_E_ARG, "%s: y_f32 = %p; a 16-byte aligned pointer is required", who, (const void*)y_f32);
    if (!aligned_to(y_bf16, 16)) return fail(c, MME_E_ARG, "%s: y_bf16 = %p; a 16-byte aligned pointer is required", who, (const void*)y_bf16);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!y_bf16 || (y_f32 && ld_y == m)) {  // the caller's f32 rows are what the row kernel reads
        Timed t(c, s, KC_CLUSTER);
        HIP_TRY(c, launch_project_rows(emb, N, d, mean, w, m, y_f32, ld_y, nullptr, 0, s));
        if (y_bf16) HIP_TRY(c, launch_normalise_rows(y_f32, N, m, y_bf16, s));
        return MME_OK;
    }
    // dense f32 rows in the workspace, in chunks of a multiple of 64 rows (every chunk is a launch of its own)
    int64_t rc = (int64_t)(workspace_cap() / ((size_t)m * 4)) / 64 * 64;
    if (rc < 64) rc = 64;
    if (rc > N) rc = N;
    int r;
    if ((r = ensure(c, c->neigh_ws, (size_t)rc * m * 4))) return r;
    float* rows = (float*)c->neigh_ws.p;
    Timed t(c, s, KC_CLUSTER);
    for (int64_t q = 0; q < N; q += rc) {
        const int64_t n = N - q < rc ? N - q : rc;
        HIP_TRY(c, launch_project_rows(emb + q * d, n, d, mean, w, m, y_f32 ? y_f32 + q * ld_y : nullptr, ld_y, rows, m, s));
        HIP_TRY(c, launch_normalise_rows(rows, n, m, y_bf16 + q * m, s));
    }
    return MME_OK;
}
