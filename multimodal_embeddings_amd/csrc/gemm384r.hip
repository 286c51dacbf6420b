// bf16 "TN" GEMM, 384 x 256 x 64 tile, 8 waves (variant 6): gemm256r.hip's kernel with a tile half as tall again, so that a
// K-tile's 1.5 x FLOP cost 80 one-KiB LDS-DMA pieces instead of 96 (-16.7 % operand bytes per FLOP through the CU's
// vector-memory path, the quantity DESIGN 4.1 found bounding the 256 x 256 kernel).
//
// 8 waves as 2 x 4, wave tile 192 x 64 = acc[12][4] of mfma_f32_16x16x32_bf16 (192 accumulator VGPRs): group 0 (waves 0-3)
// owns rows 0-191, group 1 rows 192-383, one barrier apart (ping-pong) as in the 256 x 256 kernel.  Same XOR-swizzled
// 128-byte LDS rows, same MFMA, same K order per accumulator (k-step 0 then 1 of every K-tile), same epilogues
// (gemm_epilogue.h, 12 row blocks instead of 8): outputs and LayerNorm planes are bit-identical to variant 3.
//
// Registers.  192 accumulators leave room for ONE k-step of fragments: a phase is one row third (4 row tiles) x 4 column
// tiles x one k-step = 16 MFMAs, fa[4] + fb[4] = 32 VGPRs; fb is read once per k-step, fa once per phase.  Six phases per
// K-tile, (k-step, third) = (0,0) (0,1) (0,2) (1,0) (1,1) (1,2), two barriers each.  No deferred stores (no registers).
//
// LDS.  160 KiB = ten 16-KiB slots = two K-tile buffers [A0 | A1 | A2 | B_lo | B_hi] (A part p = rows 128 p .. 128 p + 127);
// K-tile t lives in buffer t & 1.  Last reads inside K-tile t:  B phase 3 (both groups);  A0 (group 0, thirds 0 and 1)
// phase 4;  A1 phase 5 (group 0, third 2; group 1, third 0, reads it last in phase 3);  A2 (group 1) phase 5.
// Barriers: group 0's phase p is [reads | barrier 2p | MFMAs | barrier 2p+1], group 1's the same one barrier later.  A
// wave's reads of phase p have returned before its last MFMA of that phase issues, i.e. before barrier 2p+1 (group 0) or
// 2p+2 (group 1); phase 3 alone also waits lgkmcnt(0) in front of its first barrier.  A request of phase q is issued
// after barrier 2q-1 (group 0) or 2q (group 1).  So a slot may be refilled from phase p+1 on when group 0 read it last in
// phase p, from p+2 on when group 1 did, and from phase 4 on for B (phase 3's early wait).  Refill schedule, two pieces
// per wave and slot, at most one slot per phase (levelled: the same pieces as two bursts of two slots measured 3-5 % slower):
//     phase 0: A1(t+1)   phase 1: A2(t+1)   phase 2: B_hi(t+1)   phase 3: -   phase 4: B_lo(t+2)   phase 5: A0(t+2)
// (K-tile t+1's parts go to the other buffer: its B was last read in phase 3 of K-tile t-1, its A1 in phase 5 of t-1 by
// group 0, its A2 in phase 5 of t-1 by group 1, two phases before phase 1 of t.)  The stream runs on across output tiles:
// past a tile's last K-tile the requests fetch the first K-tiles of the workgroup's next tile.
//
// Counted wait.  vmcnt retires in issue order.  A slot is read one phase after the wait that covers it, that wait in front
// of its phase's first barrier (group 1 reads one barrier later than group 0 issues).  Issue order of a wave, oldest first,
// when phase 5 of K-tile t has made its request:
//     B_lo(t+1) A0(t+1) A1(t+1) A2(t+1) B_hi(t+1) | B_lo(t+2) A0(t+2)                         (2 pieces each)
// Phase 0 of K-tile t+1 reads B(t+1), A0(t+1) and A1(t+1): phase 5 waits vmcnt(4), which retires all of K-tile t+1 and
// leaves B_lo(t+2) and A0(t+2) in flight -- ONE wait per K-tile.  Every A piece has 6-7 phases to land, B_lo 7, B_hi 4
// (weights: L2 resident).  An output tile's stores enter the queue behind B_lo / A0 of the next tile's K-tile 1 and are
// retired by that tile's first phase-5 wait, five phases after the epilogue; K-tile 0 of the next tile was complete before
// the epilogue began.  The first tile's prologue establishes the same state.  Without a K-tile t+2 (the workgroup's last
// two K-tiles) phase 5 waits vmcnt(0).
//
// Epilogue operands (folded-LayerNorm epilogues 5 and 6, interior tiles).  bias and colsum depend on the column tile and
// ln_stats on the row panel, none on the K loop, so a wave requests them in compact form, one value per lane, in phase 3 of
// K-tile nk - 2 (the one phase without an LDS-DMA request): five loads into 8 VGPRs,
//     bias[n0 + 64 wn + lane]   colsum[n0 + 64 wn + lane]   ln_stats[m0 + 192 wm + 64 k + lane], k = 0..2   (float2)
// (their two lane offsets, 4 lane and 8 lane, live across the K loop as well: 10 VGPRs in all).
// In the issue order above they stand between B_hi(t+1) and B_lo(t+2), so the SAME phase-5 wait of that K-tile -- vmcnt(4),
// or vmcnt(0) without a K-tile t+2 -- retires them, two phases later; no wait count changes and the whole last K-tile lies
// between that wait and their first use.  With nk = 2 K-tile 0 is that K-tile (the prologue's requests are all older).  They
// are inline-asm loads: the compiler places no wait of its own for them, and the fast path of the epilogue holds no
// s_waitcnt vmcnt at all.  The epilogue hands every lane its columns and rows by ds_bpermute_b32 (gemm_epilogue.h,
// epilogue_wave_192x64_ln).  Edge tiles skip the loads: their guarded path loads per element as before.
// HAZARD of that form: to the compiler the eight destination registers are defined AT the asm statement.  Should it ever
// split their live ranges and copy or spill one between the load and the phase-5 wait, the copy would read a register whose
// data has not landed.  Nothing in the source forbids that; the compile gate does: profiles/gemm384_resources.txt records,
// for <5> and <6>, that between the five loads and the counted wait no instruction other than the loads names a destination
// register (today they are touched by the loads and by the epilogue's ds_bpermute_b32 alone).  Re-check it with every change
// to this file or to the compiler.
#include <type_traits>

#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_tiles.h"
#include "kernels.h"

namespace {

constexpr int TM = 384, TN = 256, TK = 64;
constexpr int SLOT = 128 * TK * 2;       // 16 KiB: 128 rows x 128 B
constexpr int KBUF = 5 * SLOT;           // A0 | A1 | A2 | B_lo | B_hi
constexpr int B_OFF = 3 * SLOT;
constexpr int LDS_BYTES = 2 * KBUF;      // 163 840
constexpr int NI = 12;                   // row blocks of a wave tile

#define S_BARRIER() asm volatile("s_barrier" ::: "memory")

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn_384r(GemmArgs g, int tiles_m, int tiles_n, int gn) {
    static_assert(epi_has_fast_path<EPI>(), "the 384-row kernel is built for the 16-byte fast-path epilogues");
    constexpr bool LN_EARLY = EPI == EPI_LN_BIAS || EPI == EPI_LN_BIAS_GELU;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fq = lane >> 4, fsw = (lane >> 1) & 7;
    const int ldb = g.K * 2;
    const int nk = g.K / TK;
    const int ntiles = tiles_m * tiles_n;

    // fragment read bases inside a K-tile buffer
    const int a_base = wm * (192 * 128) + fr * 128;
    const int b_base = B_OFF + (wn >> 1) * SLOT + ((wn & 1) * 64 + fr) * 128;
    // DMA piece geometry of this lane: pieces 2*wave, 2*wave+1 of a 128-row part
    const int pr0 = (wave * 2) * 8 + (lane >> 3), pr1 = pr0 + 8;
    char* const dst0 = lds + (wave * 2) * 1024;
    char* const dst1 = dst0 + 1024;

    struct TileCtx {
        int m0, n0, mrem, nrem;
        const char *Ag, *Wg;
    };
    auto make_ctx = [&](int tile) {  // tile order: gemm256r.hip
        TileCtx c;
        const int id = xcd_remap(tile, ntiles);
        const int gsz = tiles_m * gn;
        const int grp = id / gsz, rem = id - grp * gsz;
        const int gw = min(gn, tiles_n - grp * gn);
        const int tm_f = rem / gw, tn = grp * gn + (rem - (rem / gw) * gw);
        const int tm = g.reverse_m ? tiles_m - 1 - tm_f : tm_f;
        c.m0 = tm * TM;
        c.n0 = tn * TN;
        c.Ag = (const char*)g.A + (size_t)c.m0 * ldb;
        c.Wg = (const char*)g.W + (size_t)c.n0 * ldb;
        c.mrem = g.M - 1 - c.m0;  // rows past the matrix edge re-read the last row
        c.nrem = g.N - 1 - c.n0;
        return c;
    };
    // one 128-row part: pieces 2*wave and 2*wave+1; `rem` clamps the row, `row0` = 0 / 128 / 256.  The lane offsets are
    // recomputed per use (no VGPR lives across the MFMA phases for them)
    auto stage = [&](const char* gbase, int rem, int row0, int region) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)gbase, 0, 0x7fffffff, 0x00020000);
        const int pc0 = ((lane & 7) ^ ((pr0 >> 1) & 7)) << 4, pc1 = ((lane & 7) ^ ((pr1 >> 1) & 7)) << 4;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(dst0 + region), 16, min(pr0 + row0, rem) * ldb + pc0, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(dst1 + region), 16, min(pr1 + row0, rem) * ldb + pc1, 0, 0, 0);
    };

    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    if (g.run_if && *g.run_if == 0) return;  // device-side switch of a fallback launch (uniform)
    TileCtx cx = make_ctx(tile);
    // prologue: K-tile 0, then B_lo and A0 of K-tile 1 as phases 4 and 5 would have requested them (14 pieces per wave)
    stage(cx.Ag, cx.mrem, 0, 0);
    stage(cx.Ag, cx.mrem, 128, SLOT);
    stage(cx.Wg, cx.nrem, 0, B_OFF);
    stage(cx.Wg, cx.nrem, 128, B_OFF + SLOT);
    stage(cx.Ag, cx.mrem, 256, 2 * SLOT);
    stage(cx.Wg + TK * 2, cx.nrem, 0, KBUF + B_OFF);
    stage(cx.Ag + TK * 2, cx.mrem, 0, KBUF);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // K-tile 0 landed; B_lo and A0 of K-tile 1 in flight

    int cur = 0;  // LDS offset of the buffer of K-tile t (the other one: KBUF - cur)

    while (true) {
        const int m0 = cx.m0, n0 = cx.n0, mrem = cx.mrem, nrem = cx.nrem;
        const char* Ag = cx.Ag;
        const char* Wg = cx.Wg;
        const int next_tile = tile + gridDim.x;
        const bool has_next = next_tile < ntiles;
        const TileCtx nx = has_next ? make_ctx(next_tile) : cx;

        f32x4 acc[NI][4];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        S_BARRIER();
        if (wm == 1) S_BARRIER();  // group 1 runs one barrier behind group 0

        bf16x8 fa[4], fb[4];
        // the folded-LayerNorm epilogue's operands of this tile, one value per lane (see "Epilogue operands" above)
        [[maybe_unused]] float e_bias, e_colsum;
        [[maybe_unused]] ln_f32x2 e_st[3];
        [[maybe_unused]] const bool fast_ln = LN_EARLY && n0 + TN <= g.N && m0 + TM <= g.M;

        auto epi_fetch = [&](int t) {
            if constexpr (LN_EARLY) {
                if (t == nk - 2 && fast_ln) {  // retired by this K-tile's phase-5 wait; an edge tile loads in its guarded path
                    const float* cb = g.bias + n0 + wn * 64;
                    const float* cs = g.colsum + n0 + wn * 64;
                    const float* rp = g.ln_stats + 2 * (int64_t)(m0 + wm * 192);
                    asm volatile("global_load_dword %0, %1, %2" : "=v"(e_bias) : "v"(lane * 4), "s"(cb) : "memory");
                    asm volatile("global_load_dword %0, %1, %2" : "=v"(e_colsum) : "v"(lane * 4), "s"(cs) : "memory");
                    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(e_st[0]) : "v"(lane * 8), "s"(rp) : "memory");
                    asm volatile("global_load_dwordx2 %0, %1, %2 offset:512" : "=v"(e_st[1]) : "v"(lane * 8), "s"(rp) : "memory");
                    asm volatile("global_load_dwordx2 %0, %1, %2 offset:1024" : "=v"(e_st[2]) : "v"(lane * 8), "s"(rp) : "memory");
                }
            }
        };

#define READ_B(ks)                                                                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                         \
        fb[j] = *(const bf16x8*)(lds + cur + b_base + j * 2048 + ((((ks) * 4 + fq) ^ fsw) << 4));
#define READ_A(ks, third)                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                         \
        fa[i] = *(const bf16x8*)(lds + cur + a_base + ((third) * 4 + i) * 2048 + ((((ks) * 4 + fq) ^ fsw) << 4));
#define MFMA_THIRD(third)                                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                         \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                         \
        acc[(third) * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[(third) * 4 + i][j], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                                        \
    S_BARRIER();

#pragma nounroll  // (and no peeled first K-tile: a second instance of the body spills)
        for (int t = 0; t < nk; ++t) {
            // K-tiles t+1 / t+2 of the stream: past the end of this tile they are the next tile's first ones
            const bool nt1 = t + 1 >= nk, nt2 = t + 2 >= nk;
            const bool has1 = !nt1 || has_next, has2 = !nt2 || has_next;
            const char* w2 = nt2 ? nx.Wg + (size_t)(t + 2 - nk) * (TK * 2) : Wg + (size_t)(t + 2) * (TK * 2);
            const char* a2 = nt2 ? nx.Ag + (size_t)(t + 2 - nk) * (TK * 2) : Ag + (size_t)(t + 2) * (TK * 2);
            const char* w1 = nt1 ? nx.Wg + (size_t)(t + 1 - nk) * (TK * 2) : Wg + (size_t)(t + 1) * (TK * 2);
            const int nrem1 = nt1 ? nx.nrem : nrem;
            const char* a1 = nt1 ? nx.Ag + (size_t)(t + 1 - nk) * (TK * 2) : Ag + (size_t)(t + 1) * (TK * 2);
            const int nrem2 = nt2 ? nx.nrem : nrem, mrem2 = nt2 ? nx.mrem : mrem, mrem1 = nt1 ? nx.mrem : mrem;
            const int oth = KBUF - cur;
            /* phase 0: k-step 0, third 0 */
            READ_B(0)
            __builtin_amdgcn_sched_barrier(0);
            READ_A(0, 0)
            if (has1) stage(a1, mrem1, 128, oth + SLOT);
            S_BARRIER();
            MFMA_THIRD(0)
            /* phase 1: third 1 */
            READ_A(0, 1)
            if (has1) stage(a1, mrem1, 256, oth + 2 * SLOT);
            S_BARRIER();
            MFMA_THIRD(1)
            /* phase 2: third 2 */
            READ_A(0, 2)
            if (has1) stage(w1, nrem1, 128, oth + B_OFF + SLOT);
            S_BARRIER();
            MFMA_THIRD(2)
            /* phase 3: k-step 1, third 0 */
            READ_B(1)
            __builtin_amdgcn_sched_barrier(0);
            READ_A(1, 0)
            epi_fetch(t);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // B's last reads have returned: phase 4 refills B_lo
            S_BARRIER();
            MFMA_THIRD(0)
            /* phase 4: third 1 */
            READ_A(1, 1)
            if (has2) stage(w2, nrem2, 0, cur + B_OFF);
            S_BARRIER();
            MFMA_THIRD(1)
            /* phase 5: third 2 */
            READ_A(1, 2)
            if (has2) {
                stage(a2, mrem2, 0, cur);
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // K-tile t+1 landed; B_lo(t+2), A0(t+2) in flight
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            S_BARRIER();
            MFMA_THIRD(2)
            cur = oth;
        }
        if (wm == 0) S_BARRIER();

        // epilogue: acc[i][j][r] is C[m0 + wm*192 + i*16 + fr][n0 + wn*64 + j*16 + fq*4 + r] (rules: gemm256r.hip).
        // The lane's row / column offsets are derived HERE from a lane id the compiler cannot see through: hoisted out
        // of the tile loop they would have to live across the K loop, where no VGPR is free (they were spilled)
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int fr_e = lane_e & 15, fq_e = lane_e >> 4;
        const bool fast = n0 + TN <= g.N && m0 + TM <= g.M;
        if (fast) {
            if constexpr (LN_EARLY) {
                epilogue_wave_192x64_ln<EPI>(g, acc, m0 + wm * 192, n0 + wn * 64, fr_e, fq_e, e_bias, e_colsum, e_st);
            } else {
                epilogue_wave_128x64<EPI>(g, acc, m0 + wm * 192, n0 + wn * 64, fr_e, fq_e, [] {});
            }
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int m = m0 + wm * 192 + i * 16 + fr_e;
                if (m >= g.M) continue;
                const EpiRow er = epi_row<EPI>(m);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = n0 + wn * 64 + j * 16 + fq_e * 4;
                    if (n >= g.N) continue;
                    epi_store<EPI>(g, m, er, n, acc[i][j]);
                }
            }
        }
        if (!has_next) break;
        cx = nx;
        tile = next_tile;
    }
#undef READ_A
#undef READ_B
#undef MFMA_THIRD
}

template <int EPI>
hipError_t launch384r(const GemmArgs& g, hipStream_t s) {
    if (hipError_t e = ensure_dynamic_lds((const void*)gemm_bf16_tn_384r<EPI>, LDS_BYTES); e != hipSuccess) return e;
    const int tiles_m = (g.M + TM - 1) / TM, tiles_n = (g.N + TN - 1) / TN;
    const int ntiles = tiles_m * tiles_n;
    const int grid = ntiles < 256 ? ntiles : 256;  // one workgroup per CU
    hipLaunchKernelGGL((gemm_bf16_tn_384r<EPI>), dim3(grid), dim3(512), LDS_BYTES, s, g, tiles_m, tiles_n, gemm_column_group(g.K, tiles_n));
    return hipGetLastError();
}

}  // namespace

bool gemm384r_has(int epilogue) {
    switch (epilogue) {
        case EPI_BIAS: case EPI_BIAS_GELU: case EPI_BIAS_RES: case EPI_BIAS_RES_STATS: case EPI_LN_BIAS: case EPI_LN_BIAS_GELU: return true;
        default: return false;
    }
}

hipError_t launch_gemm384r(int epilogue, const GemmArgs& g, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    if (g.K < 2 * TK || (g.K % TK) != 0) return hipErrorInvalidValue;  // the stream looks two K-tiles ahead
    switch (epilogue) {
        case EPI_BIAS: return launch384r<EPI_BIAS>(g, s);
        case EPI_BIAS_GELU: return launch384r<EPI_BIAS_GELU>(g, s);
        case EPI_BIAS_RES: return launch384r<EPI_BIAS_RES>(g, s);
        case EPI_BIAS_RES_STATS: return launch384r<EPI_BIAS_RES_STATS>(g, s);
        case EPI_LN_BIAS: return launch384r<EPI_LN_BIAS>(g, s);
        case EPI_LN_BIAS_GELU: return launch384r<EPI_LN_BIAS_GELU>(g, s);
        default: return hipErrorInvalidValue;
    }
}
