// Multi-head self-attention of the ViT/32 @224 image towers (T = 50 tokens, dh = 64; H = 6, 12 or 16 heads), non-causal.
//
// softmax(Q K^T dh^-0.5) V with the softmax in f32.  Modelled on attention_causal.hip without the triangle; MFMA shapes,
// LDS images and the LDS-DMA idiom are those of attention.hip:
//   * One 2-wave workgroup per (crop, head) item, persistent over the items blockIdx.x, blockIdx.x + gridDim.x, ...
//     50 -> 64 rows: wave w owns the query block 32 w .. 32 w + 31 and multiplies both key tiles of 32.  K and V of an item
//     (64 rows of 128 B each, 16 KiB together) are brought by LDS-DMA, 8 pieces of 8 rows per wave, with attention.hip's
//     two source swizzles; rows 50..63 receive clamped copies of row 49 (finite whenever the input is, and never read
//     from the next item).  16 KiB of LDS and 128 threads: several workgroups share a CU and cover each other's load
//     latency, so there is no double buffer and no prefetch.
//   * EXACT row maximum, no guarded fast form.  The padded keys 50..63 are removed by SELECTION (never by adding a large
//     negative number), both in the maximum and in P: a clamped copy of key 49 counts for nothing, and whatever a padded
//     score is it reaches nothing.  P is exactly 0 there, and 0 times the clamped, finite V row is 0.
//   * Q arrives pre-multiplied by dh^-0.5 log2 e (folded into W_q / b_q at load): P = exp2(s - max).
//   * only_block = 0 or 1: only that query block is computed and stored (the pruned last layer); the other wave still
//     brings its share of K and V.  The computed block is bit-identical to the full launch: a wave's arithmetic does not
//     depend on the other wave's.
// Rounding points are attention.hip's two: P to bf16 before P.V, the output (O / sum, sum over the f32 P) to bf16.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int T50 = 50;
constexpr int ROWB = VIT_DH * 2;         // 128-byte K / V rows in LDS
constexpr int TROWS = 64;                // 2 key tiles of 32
constexpr int KV_BYTES = TROWS * ROWB;   // 8 KiB
constexpr int NPIECE = TROWS / 8;        // 8 LDS-DMA pieces of 8 rows for K, 8 for V
constexpr int NT = 2;                    // key tiles

typedef __attribute__((ext_vector_type(8))) short s16x8;

#define S_BARRIER() asm volatile("s_barrier" ::: "memory")

// the value the other half of the wave (lane ^ 32) holds: one v_permlane32_swap (attention.hip)
__device__ __forceinline__ float other_half(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float a = __uint_as_float(sw[0]), b = __uint_as_float(sw[1]);
    return (threadIdx.x & 32) ? a : b;
}

// One query block of one item: S^T = K . Q^T over both key tiles, softmax over the 50 keys, O^T = V^T . P^T, stores.
// s[kt][e] is the score of key 32 kt + (e & 3) + 8 (e >> 2) + 4 hh for this lane's query.
__device__ __forceinline__ void block_t50(const char* Kl, const char* Vl, const bf16x8 (&qf)[4], const int lane, bf16_t* op, const bool store) {
    const int r = lane & 31, hh = lane >> 5;
    const int ksw = (r >> 1) & 7;
    // transposed-read lane roles (attention.hip): group g of 16 lanes, lane 4q + p supplies row q, cols 4p..4p+3
    const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    const int vflag = (tq >> 1) & 1;
    const int v_row_off = (4 * (g >> 1) + tq) * ROWB + (16 * (g & 1) + 4 * tp) * 2;
    const int v_off0 = v_row_off + ((0 ^ vflag) << 6), v_off1 = v_row_off + ((1 ^ vflag) << 6);
    f32x16 s[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        bf16x8 kf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const bf16x8*)(Kl + (kt * 32 + r) * ROWB + (((2 * ks + hh) ^ ksw) << 4));
        f32x16 a;
#pragma unroll
        for (int e = 0; e < 16; ++e) a[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], a, 0, 0, 0);
        s[kt] = a;
    }
    // key 32 + j of the second tile is a token when 32 + j < 50
    auto real_key = [&](int e) { return 32 + (e & 3) + 8 * (e >> 2) + 4 * hh < T50; };
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[0][e]);
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, real_key(e) ? s[1][e] : -INFINITY);
    mx = fmaxf(mx, other_half(mx));  // the first tile holds 32 tokens: mx is a score
    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[0][e] = o[1][e] = 0.f;
    float sum = 0.f;
#pragma unroll
    for (int I = 0; I < 2 * NT; ++I) {  // 16 keys a step
        const int kt = I >> 1;
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = 8 * (I & 1) + j;
            float pv = __builtin_amdgcn_exp2f(s[kt][e] - mx);
            if (kt == 1) pv = real_key(e) ? pv : 0.f;
            sum += pv;
            pf[j] = (bf16_t)pv;
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const char* va = Vl + I * 16 * ROWB + (db ? v_off1 : v_off0);
            const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)va);
            const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(va + 8 * ROWB));
            const s16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), pf, o[db], 0, 0, 0);
        }
    }
    sum += other_half(sum);
    const float inv = __builtin_amdgcn_rcpf(sum);
    // o[db][4 rg + j] = O[q][32 db + 8 rg + 4 hh + j]: pair the lane halves into 16-byte stores (attention.hip)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int rp = 0; rp < 4; rp += 2) {
            bf16x4 t0, t1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t0[j] = (bf16_t)(o[db][rp * 4 + j] * inv);
                t1[j] = (bf16_t)(o[db][(rp + 1) * 4 + j] * inv);
            }
            const uint2 u0 = __builtin_bit_cast(uint2, t0), u1 = __builtin_bit_cast(uint2, t1);
            const auto ax = __builtin_amdgcn_permlane32_swap(u0.x, u1.x, false, false);
            const auto ay = __builtin_amdgcn_permlane32_swap(u0.y, u1.y, false, false);
            const uint4 w = make_uint4(ax[0], ay[0], ax[1], ay[1]);
            if (store) *(uint4*)(op + db * 32 + (rp + hh) * 8) = w;
        }
}

// qkv [n * 50, 3 * 64 H] (Q | K | V, Q pre-scaled) -> out [n * 50, 64 H]; items = n * H
__global__ __launch_bounds__(128) void attn_fwd_t50(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int items, const int H,
                                                    const int only_block) {
    __shared__ __attribute__((aligned(16))) char lds[2 * KV_BYTES];  // K | V of the current item
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = H * VIT_DH;
    const size_t qkv_ld = (size_t)3 * D * 2;  // bytes per row of the fused activation
    const int q = wave * 32 + (lane & 31), hh = lane >> 5;
    const int qc = min(q, T50 - 1);
    const bool mine = only_block < 0 || only_block == wave;  // wave-uniform
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int crop = it / H, h = it - crop * H;
        const char* hb = (const char*)qkv + (size_t)crop * T50 * qkv_ld + h * ROWB;
        if (it != (int)blockIdx.x) S_BARRIER();  // both waves are done with the previous item's K / V
        // 16 pieces of 8 rows x 128 B: wave w requests pieces w, w + 2, ...; both swizzles are applied to the source address
        for (int p = wave; p < 2 * NPIECE; p += 2) {
            const bool isv = p >= NPIECE;
            const int pp = isv ? p - NPIECE : p;
            const int row = pp * 8 + (lane >> 3);
            const int slot = lane & 7;
            const int chunk = isv ? (slot ^ (((row >> 1) & 1) << 2)) : (slot ^ ((row >> 1) & 7));
            const char* src = hb + (size_t)min(row, T50 - 1) * qkv_ld + (isv ? 2 : 1) * D * 2 + chunk * 16;
            const unsigned dst = (unsigned)(size_t)(LDS_AS char*)(lds + (isv ? KV_BYTES : 0) + pp * 1024);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst))
                         : "memory");
        }
        bf16x8 qf[4];
        {
            const char* qp = hb + (size_t)qc * qkv_ld + hh * 16;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 32);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces have landed
        S_BARRIER();                                                  // everybody's
        bf16_t* op = out + ((size_t)crop * T50 + qc) * D + h * VIT_DH;
        if (mine) block_t50(lds, lds + KV_BYTES, qf, lane, op, q < T50);
    }
}

}  // namespace

hipError_t launch_attention_t50(const void* qkv, void* out, int n, int heads, hipStream_t s, int only_block) {
    if (heads != 6 && heads != 12 && heads != 16) return hipErrorInvalidValue;  // widths 384, 768, 1024
    if (only_block < -1 || only_block > 1) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t items = (int64_t)n * heads;
    if (items > 0x7fffffff) return hipErrorInvalidValue;
    const int grid = items < 1024 ? (int)items : 1024;  // persistent: up to four workgroups per CU walk the items
    hipLaunchKernelGGL(attn_fwd_t50, dim3(grid), dim3(128), 0, s, (const bf16_t*)qkv, (bf16_t*)out, (int)items, heads, only_block);
    return hipGetLastError();
}
