// C ABI of K19 (include/mme.h, mme_hierarchy_*): argument checks and the host pass, K18's (capi_density.hip) with full rows --
// the cosine block of a chunk of rows against ALL columns, through the GEMM into the K12 workspace, then hier_core or
// hier_scan over it.  The core pass and every round's scan take the operands through the same GEMM kernel.
#include <cstdlib>

#include "ctx.h"
#include "hierarchy.h"

namespace {

int check_state(mme_ctx* c, const char* who, const mme_hierarchy_state* st, int N) {
    if (!st) return fail(c, MME_E_ARG, "%s: state is null", who);
    if (N < 0) return fail(c, MME_E_ARG, "%s: N = %d is negative", who, N);
    if (!st->core) return fail(c, MME_E_ARG, "%s: state.core is null", who);
    if (!st->comp) return fail(c, MME_E_ARG, "%s: state.comp is null", who);
    if (!st->row_key) return fail(c, MME_E_ARG, "%s: state.row_key is null", who);
    if (!st->parent) return fail(c, MME_E_ARG, "%s: state.parent is null", who);
    if (!st->comp_weight) return fail(c, MME_E_ARG, "%s: state.comp_weight is null", who);
    if (!st->comp_edge) return fail(c, MME_E_ARG, "%s: state.comp_edge is null", who);
    if (N > 1 && !st->edges) return fail(c, MME_E_ARG, "%s: state.edges is null", who);
    if (N > 1 && !st->weights) return fail(c, MME_E_ARG, "%s: state.weights is null", who);
    if (!st->counters) return fail(c, MME_E_ARG, "%s: state.counters is null", who);
    if (((uintptr_t)st->core & 15) != 0) return fail(c, MME_E_ARG, "%s: state.core = %p is not 16-byte aligned", who, (void*)st->core);
    if (((uintptr_t)st->comp & 15) != 0) return fail(c, MME_E_ARG, "%s: state.comp = %p is not 16-byte aligned", who, (void*)st->comp);
    return MME_OK;
}

HierState device_state(const mme_hierarchy_state* st) {
    HierState d{};
    d.core = st->core;
    d.comp = st->comp;
    d.row_key = (unsigned long long*)st->row_key;
    d.parent = st->parent;
    d.comp_weight = st->comp_weight;
    d.comp_edge = (unsigned long long*)st->comp_edge;
    d.edges = st->edges;
    d.weights = st->weights;
    d.counters = (unsigned long long*)st->counters;
    return d;
}

// one pass over the rows [row0, row0 + nrows) against every column: the core pass (k = min_samples - 1 >= 1), or with k = 0
// one round's scan
int pass(mme_ctx* c, const char* who, const uint16_t* emb, int N, int d, const int32_t* group, int k, int row0, int nrows,
         const mme_hierarchy_state* st, void* stream) {
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const HierState ds = device_state(st);

    // K18's chunks with full rows: rows [q, q + m) against columns [0, N); at most MME_NEIGH_WS_MB of f32 per chunk, whole
    // 256-row GEMM tiles
    static const int64_t ws_mb = getenv("MME_NEIGH_WS_MB") ? atoll(getenv("MME_NEIGH_WS_MB")) : 2048;
    const int64_t ld = ((int64_t)N + 3) & ~(int64_t)3;
    int64_t rc = (ws_mb << 20) / (ld * 4);
    rc = rc < 256 ? 256 : (rc / 256) * 256;
    const int end = row0 + nrows;
    const int64_t most = end - row0 < rc ? end - row0 : rc;
    int r;
    if ((r = ensure(c, c->neigh_ws, (size_t)most * ld * 4))) return r;
    float* block = (float*)c->neigh_ws.p;
    for (int q = row0; q < end;) {
        const int m = (int)(end - q < rc ? end - q : rc);
        GemmArgs g{};
        g.A = emb + (size_t)q * d; g.W = emb; g.M = m; g.N = N; g.K = d; g.outf = block; g.ldf = ld;
        {
            Timed t(c, s, KC_COS);
            HIP_TRY(c, launch_gemm(EPI_F32, g, s, c->gemm_variant));
        }
        Timed t(c, s, KC_NEIGH);
        if (k > 0)
            HIP_TRY(c, launch_hier_core(block, ld, m, N, q, group, k, ds, s));
        else
            HIP_TRY(c, launch_hier_scan(block, ld, m, N, q, group, ds, s));
        q += m;
    }
    return MME_OK;
}

int check_table(mme_ctx* c, const char* who, const uint16_t* emb, int N, int d, int row0, int nrows) {
    if (d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; d %% 64 == 0 is required", who, d);
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > N) return fail(c, MME_E_ARG, "%s: rows [row0 = %d, row0 + nrows = %lld) are outside 0..N = %d", who, row0, (long long)row0 + nrows, N);
    if (nrows > 0 && !emb) return fail(c, MME_E_ARG, "%s: emb is null", who);
    return MME_OK;
}

}  // namespace

int mme_hierarchy_init(mme_ctx* c, const mme_hierarchy_state* st, int N, void* stream) {
    if (!c) return MME_E_ARG;
    int r;
    if ((r = check_state(c, "mme_hierarchy_init", st, N))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_hier_init(device_state(st), N, (hipStream_t)stream));
    return MME_OK;
}

int mme_hierarchy_core(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, int min_samples, int row0, int nrows,
                       const mme_hierarchy_state* st, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_hierarchy_core";
    int r;
    if ((r = check_state(c, who, st, N))) return r;
    if (min_samples < 1) return fail(c, MME_E_ARG, "%s: min_samples = %d; at least 1 is required", who, min_samples);
    if ((r = check_table(c, who, emb, N, d, row0, nrows))) return r;
    if (nrows == 0) return MME_OK;
    if (min_samples == 1 || N < 2) {  // no selection: above every cosine, or a row without any partner
        HIP_TRY(c, hipSetDevice(c->device));
        Timed t(c, (hipStream_t)stream, KC_NEIGH);
        HIP_TRY(c, launch_hier_fill_core(device_state(st), row0, nrows, min_samples == 1 ? 1.5f : -2.0f, (hipStream_t)stream));
        return MME_OK;
    }
    return pass(c, who, emb, N, d, group, min_samples - 1, row0, nrows, st, stream);
}

int mme_hierarchy_scan(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, int row0, int nrows, const mme_hierarchy_state* st,
                       void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_hierarchy_scan";
    int r;
    if ((r = check_state(c, who, st, N))) return r;
    if ((r = check_table(c, who, emb, N, d, row0, nrows))) return r;
    if (nrows == 0 || N < 2) return MME_OK;
    return pass(c, who, emb, N, d, group, 0, row0, nrows, st, stream);
}

int mme_hierarchy_merge(mme_ctx* c, const mme_hierarchy_state* st, int N, void* stream) {
    if (!c) return MME_E_ARG;
    int r;
    if ((r = check_state(c, "mme_hierarchy_merge", st, N))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, launch_hier_merge(device_state(st), N, s));
    return MME_OK;
}
