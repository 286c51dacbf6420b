// C ABI of K18 (include/mme.h, mme_density_*): argument checks and the host pass, K14's (capi_duplicates.hip) -- the cosine
// block of a chunk of rows against the columns from the chunk's first row on, through the GEMM into the K12 workspace, then
// den_count or den_link over it.  Both passes take the same chunks of the same operands through the same GEMM kernel.
#include <cmath>
#include <cstdlib>

#include "ctx.h"
#include "density.h"

namespace {

int check_state(mme_ctx* c, const char* who, const mme_density_state* st, int N) {
    if (!st) return fail(c, MME_E_ARG, "%s: state is null", who);
    if (N < 0) return fail(c, MME_E_ARG, "%s: N = %d is negative", who, N);
    if (!st->count) return fail(c, MME_E_ARG, "%s: state.count is null", who);
    if (!st->parent) return fail(c, MME_E_ARG, "%s: state.parent is null", who);
    if (!st->border) return fail(c, MME_E_ARG, "%s: state.border is null", who);
    if (!st->counters) return fail(c, MME_E_ARG, "%s: state.counters is null", who);
    return MME_OK;
}

DenState device_state(const mme_density_state* st) {
    DenState d{};
    d.count = st->count;
    d.parent = st->parent;
    d.border = (unsigned long long*)st->border;
    d.counters = (unsigned long long*)st->counters;
    return d;
}

// one pass over the pairs (i, j), row0 <= i < row0 + nrows, i < j < N: the count pass, or under `link` the link pass
int pass(mme_ctx* c, const char* who, const uint16_t* emb, int N, int d, const int32_t* group, float min_sim, int min_samples, bool link,
         int row0, int nrows, const mme_density_state* st, void* stream) {
    int r;
    if ((r = check_state(c, who, st, N))) return r;
    if (d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; d %% 64 == 0 is required", who, d);
    if (std::isnan(min_sim)) return fail(c, MME_E_ARG, "%s: min_sim is NaN", who);
    if (link && min_samples < 1) return fail(c, MME_E_ARG, "%s: min_samples = %d; at least 1 is required", who, min_samples);
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > N) return fail(c, MME_E_ARG, "%s: rows [row0 = %d, row0 + nrows = %lld) are outside 0..N = %d", who, row0, (long long)row0 + nrows, N);
    if (nrows == 0) return MME_OK;
    if (!emb) return fail(c, MME_E_ARG, "%s: emb is null", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const DenState ds = device_state(st);

    // K14's chunks: rows [q, q + m) against columns [c0, N), c0 = q rounded down to 4; at most MME_NEIGH_WS_MB of f32 per chunk,
    // whole 256-row GEMM tiles
    static const int64_t ws_mb = getenv("MME_NEIGH_WS_MB") ? atoll(getenv("MME_NEIGH_WS_MB")) : 2048;
    struct Chunk {
        int q, m, c0, cols;
        int64_t ld;
    };
    std::vector<Chunk> chunks;
    size_t total = 0;
    const int end = row0 + nrows;
    for (int q = row0; q < end;) {
        Chunk k;
        k.q = q;
        k.c0 = q & ~3;
        k.cols = N - k.c0;
        k.ld = ((int64_t)k.cols + 3) & ~(int64_t)3;
        int64_t rc = (ws_mb << 20) / (k.ld * 4);
        rc = rc < 256 ? 256 : (rc / 256) * 256;
        k.m = (int)(end - q < rc ? end - q : rc);
        const size_t bytes = (size_t)k.m * k.ld * 4;
        if (bytes > total) total = bytes;
        chunks.push_back(k);
        q += k.m;
    }
    if ((r = ensure(c, c->neigh_ws, total))) return r;
    float* block = (float*)c->neigh_ws.p;
    for (const Chunk& k : chunks) {
        if (k.q + 1 >= N) break;  // the last row has no partner behind it
        GemmArgs g{};
        g.A = emb + (size_t)k.q * d; g.W = emb + (size_t)k.c0 * d; g.M = k.m; g.N = k.cols; g.K = d; g.outf = block; g.ldf = k.ld;
        {
            Timed t(c, s, KC_COS);
            HIP_TRY(c, launch_gemm(EPI_F32, g, s, c->gemm_variant));
        }
        Timed t(c, s, KC_NEIGH);
        if (link)
            HIP_TRY(c, launch_den_link(block, k.ld, k.m, k.cols, k.q, k.c0, group, min_sim, min_samples, ds, s));
        else
            HIP_TRY(c, launch_den_count(block, k.ld, k.m, k.cols, k.q, k.c0, group, min_sim, ds, s));
    }
    return MME_OK;
}

}  // namespace

int mme_density_init(mme_ctx* c, const mme_density_state* st, int N, void* stream) {
    if (!c) return MME_E_ARG;
    int r;
    if ((r = check_state(c, "mme_density_init", st, N))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_den_init(device_state(st), N, (hipStream_t)stream));
    return MME_OK;
}

int mme_density_count(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, float min_sim, int row0, int nrows,
                      const mme_density_state* st, void* stream) {
    if (!c) return MME_E_ARG;
    return pass(c, "mme_density_count", emb, N, d, group, min_sim, 0, false, row0, nrows, st, stream);
}

int mme_density_link(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, float min_sim, int min_samples, int row0, int nrows,
                     const mme_density_state* st, void* stream) {
    if (!c) return MME_E_ARG;
    return pass(c, "mme_density_link", emb, N, d, group, min_sim, min_samples, true, row0, nrows, st, stream);
}

int mme_density_finish(mme_ctx* c, const mme_density_state* st, int N, int min_samples, int32_t* labels, int32_t* kind, int32_t* border_idx,
                       float* border_sim, int64_t* summary, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_density_finish";
    int r;
    if ((r = check_state(c, who, st, N))) return r;
    if (min_samples < 1) return fail(c, MME_E_ARG, "%s: min_samples = %d; at least 1 is required", who, min_samples);
    if (!summary) return fail(c, MME_E_ARG, "%s: summary is null", who);
    if (N > 0 && !labels) return fail(c, MME_E_ARG, "%s: labels is null", who);
    if (N > 0 && !kind) return fail(c, MME_E_ARG, "%s: kind is null", who);
    if (N > 0 && !border_idx) return fail(c, MME_E_ARG, "%s: border_idx is null", who);
    if (N > 0 && !border_sim) return fail(c, MME_E_ARG, "%s: border_sim is null", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the label histogram: int32 [N] at the head of the K12 workspace (the cosine block of a pass enqueued before is consumed
    // by then, the next pass on this stream comes after)
    if (N > 0 && (r = ensure(c, c->neigh_ws, (size_t)N * sizeof(int32_t)))) return r;
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, launch_den_finish(device_state(st), N, min_samples, labels, kind, border_idx, border_sim, (long long*)summary, (int32_t*)c->neigh_ws.p, s));
    return MME_OK;
}
