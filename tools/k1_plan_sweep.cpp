// K1's host planning code (multimodal_embeddings_amd/csrc/k1_plan.h) over the whole admitted domain, for running under a
// sanitizer.  A stand-alone host program: it opens no device, loads nothing into another process and needs no preloaded
// runtime.  Build and run from the repository root (the host pass only; no device code is generated):
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/k1_plan_sweep.cpp -o k1_plan_sweep -lpthread && ./k1_plan_sweep
//
// What it does, for fit-and-pad, the six resize specs of tests/k1_plan_reference.py and tiles at (560, 4), one thread per rule:
//   1. every (h, w) in 1..8000 x 1..8000, a row of 8000 widths per batch, through k1_plan_records -- the functions the entry
//      points plan with -- the bands counted, not listed (listing them is 64 M sizes x ~1000 bands per rule);
//   2. the band loop itself, with its vectors, on a lattice of 1.9 M sizes per rule (every 5th height, every 7th width,
//      the edges 1..8 and 7993..8000 of both) and on 4000 random batches of 1..64 mixed sizes: every band list must cover
//      its crop's source rows once and in order.
// The limits are plain checks that abort: no refusal, LDS requests within 160 KiB, kv within the vertical pass's 160 taps,
// the window of a spec inside the crop, offsets 16-byte aligned and contiguous, totals equal to the sums.
// Exit status 0 and "clean" on the last line: nothing was reported.  (Not a pytest test: tests/test_k1_plan_cpu.py checks the
// same plan against an independent reference; this program is for the sanitizer.)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../multimodal_embeddings_amd/csrc/k1_plan.h"

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                      \
            std::fprintf(stderr, "\n");                             \
            std::abort();                                           \
        }                                                           \
    } while (0)

namespace {

struct Rule {
    const char* name;
    mme_k1_rule rule;
};

const Rule kRules[] = {
    {"fit_pad", {MME_K1_RULE_FIT_PAD, {0, 0, 0, 0}, 0, 0}},
    {"clip", {MME_K1_RULE_SPEC, {MME_RESIZE_MODE_SHORTEST_EDGE, 224, 0, 3}, 0, 0}},
    {"edge256_bicubic", {MME_K1_RULE_SPEC, {MME_RESIZE_MODE_SHORTEST_EDGE, 256, 0, 3}, 0, 0}},
    {"exact224_bilinear", {MME_K1_RULE_SPEC, {MME_RESIZE_MODE_EXACT, 224, 224, 2}, 0, 0}},
    {"edge512_bicubic", {MME_K1_RULE_SPEC, {MME_RESIZE_MODE_SHORTEST_EDGE, 512, 0, 3}, 0, 0}},
    {"exact512_bicubic", {MME_K1_RULE_SPEC, {MME_RESIZE_MODE_EXACT, 512, 512, 3}, 0, 0}},
    {"tiles560", {MME_K1_RULE_TILES, {0, 0, 0, 0}, 560, 4}},
};

// the limits of one planned batch; `listed`: the plan holds the band lists
void check_batch(const Rule& R, const std::vector<int32_t>& hw, const std::vector<mme_k1_record>& rec, const K1Plan& p, bool listed) {
    const int n = (int)rec.size();
    const bool spec = R.rule.kind == MME_K1_RULE_SPEC, tiles = R.rule.kind == MME_K1_RULE_TILES;
    int64_t tab = 0, tmp = 0, bands = 0;
    int kv_max = 0;
    for (int i = 0; i < n; ++i) {
        const mme_k1_record& r = rec[i];
        const int h = hw[2 * i], w = hw[2 * i + 1];
        CHECK(r.refused == MME_K1_OK, "%s: %d x %d refused with code %d", R.name, h, w, r.refused);
        CHECK(r.new_h >= 1 && r.new_w >= 1, "%s: %d x %d becomes %d x %d", R.name, h, w, r.new_h, r.new_w);
        CHECK(r.h_pass == (r.new_w != w) && r.v_pass == (r.new_h != h), "%s: %d x %d passes", R.name, h, w);
        CHECK(r.h_lds <= K1_LDS_LIMIT, "%s: %d x %d asks for %d bytes of LDS", R.name, h, w, r.h_lds);
        CHECK(r.kv % 4 == 0, "%s: %d x %d kv %d", R.name, h, w, r.kv);
        if (!tiles) CHECK(r.kv <= MAX_TAPS && r.v_lds <= K1_LDS_LIMIT - 16 * 1024, "%s: %d x %d kv %d, %d bytes", R.name, h, w, r.kv, r.v_lds);
        if (tiles) CHECK(r.th >= 1 && r.tw >= 1 && r.th * r.tw <= R.rule.max_tiles && r.new_h <= r.th * R.rule.tile && r.new_w <= r.tw * R.rule.tile, "%s: %d x %d grid", R.name, h, w);
        if (spec) {
            CHECK(r.r0 >= 0 && r.nr >= 1 && r.r0 + r.nr <= h, "%s: %d x %d rows [%d, +%d)", R.name, h, w, r.r0, r.nr);
            CHECK(r.top >= 0 && r.left >= 0 && r.top + VIT_IMG <= r.new_h && r.left + VIT_IMG <= r.new_w, "%s: %d x %d window", R.name, h, w);
        }
        if (r.h_class >= 0) {
            CHECK(r.h_class <= 2 && r.band_rows >= 4 && r.band_rows <= 64 && r.n_bands >= 1, "%s: %d x %d bands", R.name, h, w);
            CHECK(r.h_class == 0 ? r.band_rows % 8 == 0 : r.band_rows == 4, "%s: %d x %d rows per band %d", R.name, h, w, r.band_rows);
        }
        CHECK(r.tab_bytes % 16 == 0 && r.tmp_bytes % 16 == 0 && (r.tab_bytes > 0) == (r.h_pass || r.v_pass || spec), "%s: %d x %d bytes", R.name, h, w);
        CHECK(r.tab_off == tab && (r.tmp_bytes == 0 || r.tmp_off == tmp), "%s: %d x %d offsets", R.name, h, w);
        tab += r.tab_bytes;
        tmp += r.tmp_bytes;
        bands += r.n_bands;
        if (r.kv > kv_max) kv_max = r.kv;
    }
    CHECK((int64_t)p.tab_bytes == tab && (int64_t)p.tmp_bytes == tmp && (int64_t)p.nbands == bands && p.kv_max == kv_max, "%s: totals", R.name);
    for (int k = 0; k < 3; ++k) CHECK(k1_h_lds_request(p.lds[k]) <= (size_t)K1_LDS_LIMIT, "%s: class %d asks for %d bytes", R.name, k, p.lds[k]);
    if (!listed) return;
    // every band list covers its crop's source rows once and in order
    std::vector<int> next(n), seen(n, 0);
    for (int i = 0; i < n; ++i) next[i] = spec ? rec[i].r0 : 0;
    size_t total = 0;
    for (int k = 0; k < 3; ++k) {
        total += p.work[k].size();
        for (const HWork& wk : p.work[k]) {
            CHECK(wk.crop >= 0 && wk.crop < n, "%s: band of crop %d", R.name, wk.crop);
            const mme_k1_record& r = rec[wk.crop];
            CHECK(r.h_class == k && wk.row0 == next[wk.crop] && wk.nrows >= 1 && wk.nrows <= r.band_rows, "%s: crop %d band at row %d", R.name, wk.crop, wk.row0);
            next[wk.crop] += wk.nrows;
            ++seen[wk.crop];
        }
    }
    CHECK(total == p.nbands, "%s: %zu bands listed, %zu counted", R.name, total, p.nbands);
    for (int i = 0; i < n; ++i) {
        const int first = spec ? rec[i].r0 : 0, rows = rec[i].h_class < 0 ? 0 : (spec ? rec[i].nr : hw[2 * i]);
        CHECK(seen[i] == rec[i].n_bands && next[i] == first + rows, "%s: crop %d (%d x %d) rows covered to %d", R.name, i, hw[2 * i], hw[2 * i + 1], next[i]);
    }
}

void plan_and_check(const Rule& R, const std::vector<int32_t>& hw, std::vector<mme_k1_record>& rec, bool list) {
    const int n = (int)(hw.size() / 2);
    rec.resize(n);
    K1Plan p;
    p.list_bands = list;
    k1_plan_records(R.rule, hw.data(), n, rec.data(), p);
    check_batch(R, hw, rec, p, list);
}

void sweep_rule(const Rule* Rp) {
    const Rule& R = *Rp;
    std::vector<int32_t> hw(2 * 8000);
    std::vector<mme_k1_record> rec;
    for (int h = 1; h <= 8000; ++h) {  // 1. the whole domain, bands counted
        for (int w = 1; w <= 8000; ++w) {
            hw[2 * (w - 1)] = h;
            hw[2 * (w - 1) + 1] = w;
        }
        plan_and_check(R, hw, rec, false);
    }
    std::vector<int> axis;  // 2. the band loop on a lattice ...
    for (int v = 1; v <= 8000; ++v)
        if (v <= 8 || v >= 7993 || v % 5 == 0) axis.push_back(v);
    std::vector<int> waxis;
    for (int v = 1; v <= 8000; ++v)
        if (v <= 8 || v >= 7993 || v % 7 == 0) waxis.push_back(v);
    for (int h : axis) {
        hw.clear();
        for (int w : waxis) {
            hw.push_back(h);
            hw.push_back(w);
        }
        plan_and_check(R, hw, rec, true);
    }
    std::mt19937 rng(61);  // ... and on random batches of mixed sizes
    std::uniform_int_distribution<int> count(1, 64), any(1, 8000), small(1, 300), coin(0, 9);
    for (int b = 0; b < 4000; ++b) {
        const int n = count(rng);
        hw.clear();
        for (int i = 0; i < 2 * n; ++i) hw.push_back(coin(rng) < 3 ? small(rng) : any(rng));
        plan_and_check(R, hw, rec, true);
    }
    std::printf("%s: 64000000 sizes, %zu x %zu listed, 4000 random batches\n", R.name, axis.size(), waxis.size());
}

}  // namespace

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> threads;
    for (const Rule& R : kRules) threads.emplace_back(sweep_rule, &R);
    for (std::thread& t : threads) t.join();
    std::printf("clean, %.0f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
