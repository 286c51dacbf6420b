// Multi-head self-attention at 257 tokens (dh = 64): the ViT/14 @224 image towers (DINOv2; H = 6, 12 or 16 heads),
// softmax(Q K^T dh^-0.5) V without a mask.  MFMA shapes, LDS images and the LDS-DMA idiom are those of attention.hip
// (attention_common.h); the block routine is attention_short.hip's at nine key tiles.
//   * 257 -> 288 rows: nine key tiles of 32, nine query blocks of 32.  The last key tile holds ONE real key (256), the last
//     query block ONE real query.
//   * One workgroup of FOUR waves per (crop, head) item, persistent over the items blockIdx.x, blockIdx.x + gridDim.x, ...
//     K and V of an item are 2 x 288 rows of 128 B = 72 KiB of LDS: two workgroups share a CU's 160 KiB and cover each
//     other's load latency, so there is no double buffer.  The 72 LDS-DMA pieces of 8 rows go round the four waves, 18 each;
//     the rows past 256 receive clamped copies of row 256 (finite whenever the input is, never read from the next item).
//   * A query block keeps its nine score tiles in registers (144 accumulators a lane), so a wave owns ONE block at a time
//     and walks the blocks wave, wave + 4, wave + 8: waves 1..3 two blocks, wave 0 three (the third is the lone last block).
//     __launch_bounds__(256, 2) holds the kernel to 256 registers a lane: the eight waves of two workgroups fit a CU.
//     The Q fragment of the wave's next block is fetched before the current block is multiplied.
//   * EXACT row maximum in f32 over the 257 keys, no guarded fast form (the guard words of a pass stay zero).  The padded
//     keys 257..287 are removed by SELECTION (never by adding a large negative number), in the maximum and in P: whatever
//     such a score is -- inf or NaN from large finite K rows included -- it reaches nothing.  P is exactly 0 there, and the
//     last 16 keys (272..287, all padded) are not multiplied at all.
//   * Q arrives pre-multiplied by dh^-0.5 log2 e (folded into W_q / b_q at load): P = exp2(s - max).
//   * only_block in 0..8: only that query block is computed and stored (the pruned last layer), by wave only_block % 4; the
//     other waves still bring their share of K and V.  The block is bit-identical to the full launch: a block's arithmetic
//     is one routine on the item's K / V and its own Q rows.
// Rounding points are attention.hip's two: P to bf16 before P.V, the output (O / sum, sum over the f32 P) to bf16.
#include "attention_common.h"
#include "kernels.h"

namespace {

constexpr int MID_T = 257;
constexpr int MID_NT = (MID_T + 31) / 32;            // 9 key tiles, 9 query blocks
constexpr int MID_WAVES = 4;
constexpr int MID_KV_BYTES = MID_NT * 32 * ATTN_ROWB;  // 36 864
constexpr int MID_NPIECE = MID_NT * 4;                 // LDS-DMA pieces of 8 rows for K, as many for V
constexpr int MID_LDS = 2 * MID_KV_BYTES;              // 73 728

// One query block of one item: S^T = K . Q^T over the nine key tiles, softmax, O^T = V^T . P^T, stores.
// s[kt][e] is the score of key 32 kt + (e & 3) + 8 (e >> 2) + 4 hh for this lane's query.
__device__ __forceinline__ void mid_block(const char* Kl, const char* Vl, const bf16x8 (&qf)[4], const int lane, bf16_t* op, const bool store) {
    const int r = lane & 31, hh = lane >> 5;
    const int ksw = (r >> 1) & 7;
    const int v_off0 = vt_lane_off(lane, 0), v_off1 = vt_lane_off(lane, 1);
    constexpr int NT = MID_NT;
    f32x16 s[NT];
    bf16x8 kf[2][4];  // the next tile's K fragments are read while this tile is multiplied
    read_k_frag(Kl, 0, r, hh, ksw, kf[0]);
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        if (kt + 1 < NT) read_k_frag(Kl, kt + 1, r, hh, ksw, kf[(kt + 1) & 1]);
        f32x16 a;
#pragma unroll
        for (int e = 0; e < 16; ++e) a[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kt & 1][ks], qf[ks], a, 0, 0, 0);
        s[kt] = a;
        __builtin_amdgcn_sched_barrier(0);  // two tiles' K fragments at a time: hoisted reads would not fit beside the 144 scores
    }
    // key j of the last tile is a token only when j == 0 (key 256): element 0 of the lower half of the wave
    const bool lower = hh == 0;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT - 1; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[kt][e]);
    mx = fmaxf(mx, lower ? s[NT - 1][0] : -INFINITY);
    mx = fmaxf(mx, other_half(mx));
    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[0][e] = o[1][e] = 0.f;
    float sum = 0.f;
    constexpr int NI = 2 * NT - 1;  // 16 keys a step; the step of keys 272..287 would add exact zeros
    s16x8 vf[2][2];  // the next step's V^T fragments are read while this step's P is formed
#pragma unroll
    for (int db = 0; db < 2; ++db) vf[0][db] = read_vt_frag(Vl + (db ? v_off1 : v_off0), ATTN_ROWB);
#pragma unroll
    for (int I = 0; I < NI; ++I) {
        const int kt = I >> 1;
        if (I + 1 < NI) {
#pragma unroll
            for (int db = 0; db < 2; ++db) vf[(I + 1) & 1][db] = read_vt_frag(Vl + (I + 1) * 16 * ATTN_ROWB + (db ? v_off1 : v_off0), ATTN_ROWB);
        }
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = 8 * (I & 1) + j;
            float pv = __builtin_amdgcn_exp2f(s[kt][e] - mx);
            if (kt == NT - 1) pv = (e == 0 && lower) ? pv : 0.f;
            sum += pv;
            pf[j] = (bf16_t)pv;
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf[I & 1][db]), pf, o[db], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    sum += other_half(sum);
    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int rp = 0; rp < 4; rp += 2) {
            const uint4 w = paired_o(o[db], rp, inv);
            if (store) *(uint4*)(op + db * 32 + (rp + hh) * 8) = w;
        }
}

__device__ __forceinline__ void load_q(const char* hb, const size_t qkv_ld, const int block, const int lane, bf16x8 (&qf)[4]) {
    const int qc = min(block * 32 + (lane & 31), MID_T - 1);
    const char* qp = hb + (size_t)qc * qkv_ld + (lane >> 5) * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 32);
}

// qkv [n * 257, 3 * 64 H] (Q | K | V, Q pre-scaled) -> out [n * 257, 64 H]; items = n * H
__global__ __launch_bounds__(64 * MID_WAVES, 2) void attn_mid(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int items, const int H,
                                                              const int only_block) {
    extern __shared__ __attribute__((aligned(16))) char lds[];  // K | V of the current item
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = H * VIT_DH;
    const size_t qkv_ld = (size_t)3 * D * 2;  // bytes per row of the fused activation
    // this wave's query blocks: b0, b0 + 4, ... (nblk of them); wave-uniform
    const int b0 = only_block >= 0 ? only_block : wave;
    const int nblk = only_block >= 0 ? ((only_block & (MID_WAVES - 1)) == wave ? 1 : 0) : (MID_NT - wave + MID_WAVES - 1) / MID_WAVES;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int seq = it / H, h = it - seq * H;
        const char* hb = (const char*)qkv + (size_t)seq * MID_T * qkv_ld + h * ATTN_ROWB;
        if (it != (int)blockIdx.x) S_BARRIER();  // every wave is done with the previous item's K / V
        for (int p = wave; p < 2 * MID_NPIECE; p += MID_WAVES) {  // both swizzles are applied to the source address
            const bool isv = p >= MID_NPIECE;
            const int pp = isv ? p - MID_NPIECE : p;
            lds_dma16(kv_piece_src<MID_T - 1>(hb, qkv_ld, D, isv, pp, lane), lds + (isv ? MID_KV_BYTES : 0) + pp * 1024);
        }
        bf16x8 qf[4];
        load_q(hb, qkv_ld, b0, lane, qf);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces have landed
        S_BARRIER();                                                  // everybody's
#pragma unroll 1
        for (int k = 0; k < nblk; ++k) {
            const int blk = b0 + MID_WAVES * k;
            bf16x8 qn[4];
            load_q(hb, qkv_ld, k + 1 < nblk ? blk + MID_WAVES : blk, lane, qn);  // the next block's rows (the same rows again behind the last)
            const int q = blk * 32 + (lane & 31);
            bf16_t* op = out + ((size_t)seq * MID_T + min(q, MID_T - 1)) * D + h * VIT_DH;
            mid_block(lds, lds + MID_KV_BYTES, qf, lane, op, q < MID_T);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
        }
    }
}

}  // namespace

static_assert(count_attn(ATTN_MID) == 1 && attn_row(ATTN_MID, MID_T), "attn_mid: the one layout of this family is MID_T tokens");

// behind launch_attention_exact (attention_short.hip), which has checked heads and only_block against the layout and n > 0
hipError_t launch_attn_mid(const void* qkv, void* out, int n, int heads, hipStream_t s, int only_block) {
    const int64_t items = (int64_t)n * heads;
    if (items > 0x7fffffff) return hipErrorInvalidValue;
    if (hipError_t e = ensure_dynamic_lds((const void*)attn_mid, MID_LDS); e != hipSuccess) return e;
    const int grid = items < 512 ? (int)items : 512;  // persistent: two workgroups per CU walk the items
    hipLaunchKernelGGL(attn_mid, dim3(grid), dim3(64 * MID_WAVES), MID_LDS, s, (const bf16_t*)qkv, (bf16_t*)out, (int)items, heads, only_block);
    return hipGetLastError();
}
