// C ABI of K15 (include/mme.h, mme_kmeans*): argument checks and the host pass -- the cosine of a chunk of rows against the
// centroids through the GEMM into the K12 workspace, kmeans_argmax_rows over it; the update's scratch sits in front of
// that block.  Everything is enqueued at once: the iterations past convergence are switched off on the device.
// At the end, K16 (mme_silhouette*): the update on given labels, silhouette_rows and the reductions (silhouette.hip).
#include <algorithm>
#include <cstdlib>

#include "ctx.h"
#include "kmeans.h"

namespace {

// the head of the K12 workspace during a k-means call
struct Plan {
    size_t o_rank, o_order, o_start, o_cnt, o_block, total;
    int chunk, nchunks;  // of the update
    int64_t ld;          // row pitch of the cosine block
    int rc;              // rows per assignment chunk
};
constexpr size_t CTRL_BYTES = 256;  // int go at 0, int64 moved at 8

// chunk_rows: 0 = by the workspace size (whole 256-row GEMM tiles, as K12's chunks)
Plan make_plan(int N, int k, int chunk_rows, bool with_update) {
    Plan p{};
    size_t total = CTRL_BYTES;
    auto carve = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) & ~(size_t)255; return o; };
    kmeans_plan(N, k, &p.chunk, &p.nchunks);
    if (with_update) {
        p.o_rank = carve((size_t)N * 4);
        p.o_order = carve((size_t)N * 4);
        p.o_start = carve((size_t)k * 4);
        p.o_cnt = carve((size_t)p.nchunks * k * 4);
    } else {
        p.o_order = carve((size_t)k * 4);  // the start rows of mme_kmeans with max_iter = 0
    }
    p.ld = ((int64_t)k + 3) & ~(int64_t)3;
    static const int64_t ws_mb = getenv("MME_NEIGH_WS_MB") ? atoll(getenv("MME_NEIGH_WS_MB")) : 2048;
    int64_t rc = chunk_rows > 0 ? chunk_rows : (ws_mb << 20) / (p.ld * 4);
    if (chunk_rows <= 0) rc = rc < 256 ? 256 : (rc / 256) * 256;
    if (rc > N) rc = N;
    p.rc = (int)rc;
    p.o_block = carve((size_t)rc * p.ld * 4);
    p.total = total;
    return p;
}

KmeansScratch scratch_of(const Plan& p, char* ws) {
    KmeansScratch s{};
    s.rank = (int32_t*)(ws + p.o_rank);
    s.order = (int32_t*)(ws + p.o_order);
    s.start = (int32_t*)(ws + p.o_start);
    s.cnt = (int32_t*)(ws + p.o_cnt);
    s.chunk = p.chunk;
    s.nchunks = p.nchunks;
    return s;
}

// One GEMM kernel for every chunk of a call, whatever its rows, so that the chunking never changes a bit: the 256 x 256
// kernel (which also honours run_if) from K = 128 on, the 128 x 128 kernel at K = 64 (it runs ungated into the workspace;
// the argmax behind it is gated).
int assign(mme_ctx* c, const uint16_t* emb, const uint16_t* centroids, int N, int d, int k, const Plan& p, char* ws, int32_t* labels, float* sim,
           long long* moved, const int* run_if, hipStream_t s) {
    float* block = (float*)(ws + p.o_block);
    for (int q = 0; q < N; q += p.rc) {
        const int m = N - q < p.rc ? N - q : p.rc;
        GemmArgs g{};
        g.A = emb + (size_t)q * d; g.W = centroids; g.M = m; g.N = k; g.K = d; g.outf = block; g.ldf = p.ld; g.run_if = run_if;
        {
            Timed t(c, s, KC_COS);
            HIP_TRY(c, launch_gemm(EPI_F32, g, s, d >= 128 ? 3 : 1));
        }
        Timed t(c, s, KC_CLUSTER);
        HIP_TRY(c, launch_kmeans_argmax_rows(block, p.ld, k, m, labels + q, sim + q, moved, run_if, s));
    }
    return MME_OK;
}

int check_shape(mme_ctx* c, const char* who, int N, int d, int k) {
    if (N < 1) return fail(c, MME_E_ARG, "%s: N = %d; at least one row is required", who, N);
    if (d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; d %% 64 == 0 is required", who, d);
    if (k < 1 || k > 65536 || k > N) return fail(c, MME_E_ARG, "%s: k = %d is outside 1..min(N, 65536) (N = %d)", who, k, N);
    return MME_OK;
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int mme_kmeans(mme_ctx* c, const uint16_t* emb, int N, int d, int k, const int32_t* init_rows, int max_iter, const mme_kmeans_state* st,
               void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_kmeans";
    int r;
    if (!st) return fail(c, MME_E_ARG, "%s: state is null", who);
    if ((r = check_shape(c, who, N, d, k))) return r;
    if (max_iter < 0 || max_iter > 1000) return fail(c, MME_E_ARG, "%s: max_iter = %d is outside 0..1000", who, max_iter);
    if (!emb) return fail(c, MME_E_ARG, "%s: emb is null", who);
    if (!st->centroids) return fail(c, MME_E_ARG, "%s: state.centroids is null", who);
    if (!st->sums) return fail(c, MME_E_ARG, "%s: state.sums is null", who);
    if (!st->counts) return fail(c, MME_E_ARG, "%s: state.counts is null", who);
    if (!st->labels) return fail(c, MME_E_ARG, "%s: state.labels is null", who);
    if (!st->sim) return fail(c, MME_E_ARG, "%s: state.sim is null", who);
    if (!st->info) return fail(c, MME_E_ARG, "%s: state.info is null", who);
    if (!st->objective) return fail(c, MME_E_ARG, "%s: state.objective is null", who);
    if (init_rows) {
        std::vector<int32_t> seen(init_rows, init_rows + k);
        for (int j = 0; j < k; ++j)
            if (seen[j] < 0 || seen[j] >= N) return fail(c, MME_E_ARG, "%s: init_rows[%d] = %d is outside 0..N-1 (N = %d)", who, j, seen[j], N);
        std::sort(seen.begin(), seen.end());
        for (int j = 1; j < k; ++j)
            if (seen[j] == seen[j - 1]) return fail(c, MME_E_ARG, "%s: init_rows lists row %d twice", who, seen[j]);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const Plan p = make_plan(N, k, 0, max_iter > 0);
    if ((r = ensure(c, c->neigh_ws, p.total))) return r;
    char* ws = (char*)c->neigh_ws.p;
    int* ctrl = (int*)ws;
    long long* moved = (long long*)(ws + 8);
    {
        Timed t(c, s, KC_CLUSTER);
        if (init_rows) {
            int32_t* rows_dev = (int32_t*)(ws + p.o_order);  // consumed before the first update writes `order`
            HIP_TRY(c, hipMemcpyAsync(rows_dev, init_rows, (size_t)k * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, launch_kmeans_gather_rows(emb, rows_dev, k, d, st->centroids, s));
        }
        HIP_TRY(c, hipMemsetAsync(ws, 0, CTRL_BYTES, s));
        HIP_TRY(c, launch_kmeans_fill_labels(st->labels, N, s));
    }
    if ((r = assign(c, emb, st->centroids, N, d, k, p, ws, st->labels, st->sim, moved, nullptr, s))) return r;
    {
        Timed t(c, s, KC_CLUSTER);
        HIP_TRY(c, launch_kmeans_step_end(ctrl, moved, st->sim, N, nullptr, k, (long long*)st->info, st->objective, 1, s));
    }
    const KmeansScratch sc = scratch_of(p, ws);
    for (int it = 0; it < max_iter; ++it) {
        {
            Timed t(c, s, KC_CLUSTER);
            HIP_TRY(c, launch_kmeans_update(emb, st->labels, N, d, k, st->sums, st->counts, st->centroids, sc, ctrl, s));
        }
        if ((r = assign(c, emb, st->centroids, N, d, k, p, ws, st->labels, st->sim, moved, ctrl, s))) return r;
        Timed t(c, s, KC_CLUSTER);
        HIP_TRY(c, launch_kmeans_step_end(ctrl, moved, st->sim, N, st->counts, k, (long long*)st->info, st->objective, 0, s));
    }
    return MME_OK;
}

int mme_kmeans_apply(mme_ctx* c, int op, const mme_kmeans_apply_args* a, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_kmeans_apply";
    if (!a) return fail(c, MME_E_ARG, "%s: args is null", who);
    if (op < 0 || op > 2) return fail(c, MME_E_ARG, "%s: op %d outside 0..2", who, op);
    int r;
    if (a->N < 1 || a->N > (1 << 24)) return fail(c, MME_E_ARG, "%s: N = %d outside 1..2^24", who, a->N);
    if (a->k < 1 || a->k > 65536) return fail(c, MME_E_ARG, "%s: k = %d outside 1..65536", who, a->k);
    if (a->run_if && !aligned_to(a->run_if, 4)) return fail(c, MME_E_ARG, "%s: run_if must be 4-byte aligned", who);
    if (!a->labels || !aligned_to(a->labels, 4)) return fail(c, MME_E_ARG, "%s: labels must be non-null and 4-byte aligned", who);
    if (op <= 1) {
        if (!a->sim || !aligned_to(a->sim, 4)) return fail(c, MME_E_ARG, "%s: op %d needs sim non-null and 4-byte aligned", who, op);
        if (!a->moved || !aligned_to(a->moved, 8)) return fail(c, MME_E_ARG, "%s: op %d needs moved non-null and 8-byte aligned", who, op);
    }
    if (op == MME_KMEANS_ARGMAX) {
        if ((a->ld % 4) != 0 || a->ld < a->k || a->ld > ((int64_t)1 << 30))
            return fail(c, MME_E_ARG, "%s: op 0 needs ld %% 4 == 0 and k <= ld <= 2^30 (ld = %lld, k = %d)", who, (long long)a->ld, a->k);
        if (!a->qsim || !aligned_to(a->qsim, 16)) return fail(c, MME_E_ARG, "%s: op 0 needs qsim non-null and 16-byte aligned", who);
    } else {
        if (a->d < 64 || a->d > (1 << 16) || (a->d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; a multiple of 64 in 64..65536 is required", who, a->d);
        if (!a->emb || !aligned_to(a->emb, 16)) return fail(c, MME_E_ARG, "%s: op %d needs emb non-null and 16-byte aligned", who, op);
        if (!a->centroids || !aligned_to(a->centroids, 16)) return fail(c, MME_E_ARG, "%s: op %d needs centroids non-null and 16-byte aligned", who, op);
    }
    if (op == MME_KMEANS_ASSIGN && (a->chunk_rows < 0 || a->chunk_rows > (1 << 24)))
        return fail(c, MME_E_ARG, "%s: chunk_rows = %d outside 0..2^24", who, a->chunk_rows);
    if (op == MME_KMEANS_UPDATE) {
        if (!a->sums || !aligned_to(a->sums, 8)) return fail(c, MME_E_ARG, "%s: op 2 needs sums non-null and 8-byte aligned", who);
        if (!a->counts || !aligned_to(a->counts, 4)) return fail(c, MME_E_ARG, "%s: op 2 needs counts non-null and 4-byte aligned", who);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (op == MME_KMEANS_ARGMAX) {
        Timed t(c, s, KC_CLUSTER);
        HIP_TRY(c, launch_kmeans_argmax_rows(a->qsim, a->ld, a->k, a->N, a->labels, a->sim, (long long*)a->moved, a->run_if, s));
    } else {
        const Plan p = make_plan(a->N, a->k, op == MME_KMEANS_ASSIGN ? a->chunk_rows : 0, op == MME_KMEANS_UPDATE);
        if ((r = ensure(c, c->neigh_ws, p.total))) return r;
        char* ws = (char*)c->neigh_ws.p;
        if (op == MME_KMEANS_ASSIGN) {
            if ((r = assign(c, a->emb, a->centroids, a->N, a->d, a->k, p, ws, a->labels, a->sim, (long long*)a->moved, a->run_if, s))) return r;
        } else {
            Timed t(c, s, KC_CLUSTER);
            HIP_TRY(c, launch_kmeans_update(a->emb, a->labels, a->N, a->d, a->k, a->sums, a->counts, a->centroids, scratch_of(p, ws), a->run_if, s));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return MME_OK;
}

// ---- K16: the silhouette of a partition (silhouette.hip) ----

namespace {

int check_silhouette_shape(mme_ctx* c, const char* who, int N, int d, int k) {
    if (N < 2) return fail(c, MME_E_ARG, "%s: N = %d; at least two rows are required", who, N);
    if (d <= 0 || (d % 64) != 0) return fail(c, MME_E_ARG, "%s: d = %d; d %% 64 == 0 is required", who, d);
    if (k < 2 || k > 65536 || k > N) return fail(c, MME_E_ARG, "%s: k = %d is outside 2..min(N, 65536) (N = %d)", who, k, N);
    return MME_OK;
}

}  // namespace

int mme_silhouette(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* labels, int k, const mme_silhouette_out* out, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_silhouette";
    int r;
    if (!out) return fail(c, MME_E_ARG, "%s: out is null", who);
    if ((r = check_silhouette_shape(c, who, N, d, k))) return r;
    if (!emb) return fail(c, MME_E_ARG, "%s: emb is null", who);
    if (!labels) return fail(c, MME_E_ARG, "%s: labels is null", who);
    if (!out->cluster) return fail(c, MME_E_ARG, "%s: out.cluster is null", who);
    if (!out->score) return fail(c, MME_E_ARG, "%s: out.score is null", who);
    if (!out->info) return fail(c, MME_E_ARG, "%s: out.info is null", who);
    if (!out->sums) return fail(c, MME_E_ARG, "%s: out.sums is null", who);
    if (!out->counts) return fail(c, MME_E_ARG, "%s: out.counts is null", who);
    if (!aligned_to(emb, 16)) return fail(c, MME_E_ARG, "%s: emb must be 16-byte aligned", who);
    if (!aligned_to(out->sums, 16)) return fail(c, MME_E_ARG, "%s: out.sums must be 16-byte aligned", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the head of the K12 workspace: the update's scratch, the centroids the update writes (the caller's are not ours to
    // change), the samples when the caller wants none, and the clusters' sums
    KmeansScratch sc{};
    kmeans_plan(N, k, &sc.chunk, &sc.nchunks);
    size_t total = 0;
    auto carve = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_rank = carve((size_t)N * 4), o_order = carve((size_t)N * 4), o_start = carve((size_t)k * 4);
    const size_t o_cnt = carve((size_t)sc.nchunks * k * 4), o_cen = carve((size_t)k * d * 2);
    const size_t o_samp = carve(out->sample ? 0 : (size_t)N * 8), o_csum = carve((size_t)k * 8);
    if ((r = ensure(c, c->neigh_ws, total))) return r;
    char* ws = (char*)c->neigh_ws.p;
    sc.rank = (int32_t*)(ws + o_rank);
    sc.order = (int32_t*)(ws + o_order);
    sc.start = (int32_t*)(ws + o_start);
    sc.cnt = (int32_t*)(ws + o_cnt);
    double* sample = out->sample ? out->sample : (double*)(ws + o_samp);
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, launch_kmeans_update(emb, labels, N, d, k, out->sums, out->counts, (uint16_t*)(ws + o_cen), sc, nullptr, s));
    HIP_TRY(c, launch_silhouette_rows(emb, N, d, labels, k, out->sums, out->counts, sample, s));
    HIP_TRY(c, launch_silhouette_reduce(sample, sc.order, sc.start, out->counts, k, (double*)(ws + o_csum), out->cluster, out->score,
                                        (long long*)out->info, s));
    return MME_OK;
}

int mme_silhouette_rows(mme_ctx* c, const uint16_t* emb, int N, int d, const int32_t* labels, int k, const double* sums, const int32_t* counts,
                        double* sample, void* stream) {
    if (!c) return MME_E_ARG;
    const char* who = "mme_silhouette_rows";
    int r;
    if ((r = check_silhouette_shape(c, who, N, d, k))) return r;
    if (!emb || !aligned_to(emb, 16)) return fail(c, MME_E_ARG, "%s: emb must be non-null and 16-byte aligned", who);
    if (!labels) return fail(c, MME_E_ARG, "%s: labels is null", who);
    if (!sums || !aligned_to(sums, 16)) return fail(c, MME_E_ARG, "%s: sums must be non-null and 16-byte aligned", who);
    if (!counts) return fail(c, MME_E_ARG, "%s: counts is null", who);
    if (!sample) return fail(c, MME_E_ARG, "%s: sample is null", who);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    Timed t(c, s, KC_CLUSTER);
    HIP_TRY(c, launch_silhouette_rows(emb, N, d, labels, k, sums, counts, sample, s));
    return MME_OK;
}
