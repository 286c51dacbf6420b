// C ABI of K14 (include/mme.h, mme_duplicates_*): argument checks and the host pass -- the cosine block of a chunk of rows
// against the columns from the chunk's first row on, through the GEMM into the K12 workspace, then dup_scan over it.
#include <cmath>
#include <cstdlib>

#include "ctx.h"
#include "duplicates.h"

namespace {

// the checks every call makes of a state for N rows; `who` is the entry point, `what` names the state argument
int check_state(mme_ctx* c, const char* who, const char* what, const mme_dup_state* st, int N) {
    if (!st) return fail(c, MME_E_ARG, "%s: %s is null", who, what);
    if (N < 0) return fail(c, MME_E_ARG, "%s: N = %d is negative", who, N);
    if (!st->parent) return fail(c, MME_E_ARG, "%s: %s.parent is null", who, what);
    if (!st->degree) return fail(c, MME_E_ARG, "%s: %s.degree is null", who, what);
    if (!st->best) return fail(c, MME_E_ARG, "%s: %s.best is null", who, what);
    if (!st->counters) return fail(c, MME_E_ARG, "%s: %s.counters is null", who, what);
    if (st->edge_cap < 0) return fail(c, MME_E_ARG, "%s: %s.edge_cap = %lld is negative", who, what, (long long)st->edge_cap);
    if (st->edge_cap > 0 && !st->edges) return fail(c, MME_E_ARG, "%s: %s.edges is null with edge_cap = %lld", who, what, (long long)st->edge_cap);
    if (st->edge_cap > 0 && !st->edge_sim) return fail(c, MME_E_ARG, "%s: %s.edge_sim is null with edge_cap = %lld", who, what, (long long)st->edge_cap);
    if (st->page_pairs && (st->P < 1 || st->P > 4096)) return fail(c, MME_E_ARG, "%s: %s.P = %d with page_pairs set; 1..4096 pages are supported", who, what, st->P);
    return MME_OK;
}

DupState device_state(const mme_dup_state* st) {
    DupState d{};
    d.parent = st->parent;
    d.degree = st->degree;
    d.best = (unsigned long long*)st->best;
    d.page_pairs = st->page_pairs;
    d.edges = st->edge_cap > 0 ? st->edges : nullptr;  // a list without room is no list
    d.edge_sim = st->edge_cap > 0 ? st->edge_sim : nullptr;
    d.counters = (unsigned long long*)st->counters;
    d.edge_cap = st->edge_cap;
    d.P = st->page_pairs ? st->P : 0;
    return d;
}

}  // namespace

int mme_duplicates_init(mme_ctx* c, const mme_dup_state* st, int N, void* stream) {
    if (!c) return MME_E_ARG;
    int r;
    if ((r = check_state(c, "mme_duplicates_init", "state", st, N))) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_dup_init(device_state(st), N, (hipStream_t)stream));
    return MME_OK;
}

int mme_duplicates_scan(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* group, const int32_t* page_of, float min_sim, int row0,
                        int nrows, const mme_dup_state* st, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_duplicates_scan";
    int r;
    if ((r = check_state(c, who, "state", st, N))) return r;
    if (d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; d %% 64 == 0 is required", who, d);
    if (std::isnan(min_sim)) return fail(c, MME_E_ARG, "%s: min_sim is NaN", who);
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > N) return fail(c, MME_E_ARG, "%s: rows [row0 = %d, row0 + nrows = %lld) are outside 0..N = %d", who, row0, (long long)row0 + nrows, N);
    if (st->page_pairs && !page_of) return fail(c, MME_E_ARG, "%s: page_of is null with state.page_pairs set", who);
    if (nrows == 0) return MME_OK;
    if (!emb) return fail(c, MME_E_ARG, "%s: emb is null", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const DupState ds = device_state(st);

    // Rows [q, q + m) against columns [c0, N), c0 = q rounded down to 4 (the block's rows, and the rows of emb the GEMM reads
    // as its second operand, stay 16-byte aligned).  At most 2 GiB of f32 per chunk: the triangle gets narrower as q grows,
    // so later chunks take more rows.  Whole 256-row GEMM tiles, as K12's chunks.
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
        HIP_TRY(c, launch_dup_scan(block, k.ld, k.m, k.cols, k.q, k.c0, group, page_of, min_sim, ds, s));
    }
    return MME_OK;
}

int mme_duplicates_merge(mme_ctx* c, const mme_dup_state* dst, const mme_dup_state* src, int N, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_duplicates_merge";
    int r;
    if ((r = check_state(c, who, "dst", dst, N))) return r;
    if ((r = check_state(c, who, "src", src, N))) return r;
    if (dst->parent == src->parent) return fail(c, MME_E_ARG, "%s: dst and src are the same state", who);
    if ((dst->page_pairs != nullptr) != (src->page_pairs != nullptr) || (dst->page_pairs && dst->P != src->P))
        return fail(c, MME_E_ARG, "%s: page_pairs of dst (P = %d) and src (P = %d) must both be set, with one P, or both be null", who,
                    dst->page_pairs ? dst->P : 0, src->page_pairs ? src->P : 0);
    HIP_TRY(c, hipSetDevice(c->device));
    Timed t(c, (hipStream_t)stream, KC_NEIGH);
    HIP_TRY(c, launch_dup_merge(device_state(dst), device_state(src), N, (hipStream_t)stream));
    return MME_OK;
}

int mme_duplicates_finish(mme_ctx* c, const mme_dup_state* st, int N, int32_t* labels, int32_t* best_idx, float* best_sim, int64_t* summary,
                          void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_duplicates_finish";
    int r;
    if ((r = check_state(c, who, "state", st, N))) return r;
    if (!summary) return fail(c, MME_E_ARG, "%s: summary is null", who);
    if (N > 0 && !labels) return fail(c, MME_E_ARG, "%s: labels is null", who);
    if (N > 0 && !best_idx) return fail(c, MME_E_ARG, "%s: best_idx is null", who);
    if (N > 0 && !best_sim) return fail(c, MME_E_ARG, "%s: best_sim is null", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the label histogram: int32 [N] at the head of the K12 workspace (the cosine block of a scan enqueued before is consumed
    // by then, the next scan on this stream comes after)
    if (N > 0 && (r = ensure(c, c->neigh_ws, (size_t)N * sizeof(int32_t)))) return r;
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, launch_dup_finish(device_state(st), N, labels, best_idx, best_sim, (long long*)summary, (int32_t*)c->neigh_ws.p, s));
    return MME_OK;
}
