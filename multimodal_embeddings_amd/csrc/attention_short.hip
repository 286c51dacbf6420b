// Multi-head self-attention of the short sequences (dh = 64), one kernel template over <T, CAUSAL>:
//   * <77, true>: the CLIP text tower (H = 8, 12 or 16 heads).  Restates transformers models/clip/modeling_clip.py,
//     CLIPAttention under CLIPTextTransformer's causal mask: softmax(Q K^T dh^-0.5 + mask) V with mask[i, j] = -inf for
//     j > i.  Three waves (77 -> 96 rows).
//   * <50, false>: the ViT/32 @224 image towers (H = 6, 12 or 16 heads): softmax(Q K^T dh^-0.5) V.  Two waves (50 -> 64).
//   * <64, false>: the SigLIP text tower (H = 8, 12 or 16 heads), transformers models/siglip/modeling_siglip.py,
//     SiglipAttention with no mask of any kind (pad tokens are attended).  Two waves, 16 KiB of LDS.  T is a multiple of 32:
//     there is no padded key and no clamped row -- every LDS row is a token's, kv_piece_src<63> and min(q, 63) clamp nothing,
//     counts(e) folds to true, every lane stores -- and the last row read is row 64 n - 1 of qkv.
// The softmax is in f32.  MFMA shapes, LDS images and the LDS-DMA idiom are those of attention.hip (attention_common.h);
// what differs:
//   * One workgroup of (T + 31) / 32 waves per (sequence, head) item, persistent over the items blockIdx.x, blockIdx.x +
//     gridDim.x, ...  Wave w owns the query block 32 w .. 32 w + 31.  K and V of an item (rows of 128 B each: 24 KiB at 77
//     tokens, 16 KiB at 50) are brought by LDS-DMA in pieces of 8 rows, piece p by wave p mod waves; the rows past T - 1
//     receive clamped copies of row T - 1 (finite whenever the input is, and never read from the next item).  An item is
//     so little LDS that several workgroups share a CU and cover each other's load latency: there is no double buffer and
//     no prefetch here.
//   * CAUSAL: wave w multiplies the key tiles 0..w ONLY -- the tiles wholly above the diagonal are skipped (6 of the 9
//     tile products remain) -- else every tile.
//   * EXACT row maximum over the keys that count, no guarded fast form.  Only the last tile a block multiplies holds keys
//     that do not count: key j of the diagonal tile when j > i (CAUSAL; the padded keys 77..95 are above every stored
//     query), else the padded keys T.. .  They are removed by SELECTION (never by adding a large negative number), both in
//     the maximum and in P, so whatever such a score is -- inf or NaN from large finite K rows included -- it reaches
//     nothing: P is exactly 0 there, and 0 times the clamped, finite V row is 0.
//   * Q arrives pre-multiplied by dh^-0.5 log2 e (folded into W_q / b_q at load, as for attention.hip): P = exp2(s - max).
//   * only_block >= 0 (not CAUSAL): only that query block is computed and stored (the pruned last layer); the other wave
//     still brings its share of K and V.  The computed block is bit-identical to the full launch: a wave's arithmetic does
//     not depend on the other wave's.  The causal kernel takes the argument and ignores it (its launcher passes -1).
// Rounding points are attention.hip's two: P to bf16 before P.V, the output (O / sum, sum over the f32 P) to bf16.
// Query 0 of a causal item sees one key: P = 1, sum = 1, the output is V[0] bit for bit.
#include "attention_common.h"
#include "kernels.h"

namespace {

// Query block W of one item: S^T = K . Q^T over its key tiles, softmax, O^T = V^T . P^T, stores.
// s[kt][e] is the score of key 32 kt + (e & 3) + 8 (e >> 2) + 4 hh for this lane's query 32 W + r.
template <int T, bool CAUSAL, int W>
__device__ __forceinline__ void short_block(const char* Kl, const char* Vl, const bf16x8 (&qf)[4], const int lane, bf16_t* op, const bool store) {
    const int r = lane & 31, hh = lane >> 5;
    const int ksw = (r >> 1) & 7;
    const int v_off0 = vt_lane_off(lane, 0), v_off1 = vt_lane_off(lane, 1);
    constexpr int NT = CAUSAL ? W + 1 : (T + 31) / 32;  // key tiles: at or below the diagonal, or all
    f32x16 s[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        bf16x8 kf[4];
#pragma unroll  // read_k_frag's text: through the helper one operand pair of the address arithmetic comes out swapped
        for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const bf16x8*)(Kl + (kt * 32 + r) * ATTN_ROWB + (((2 * ks + hh) ^ ksw) << 4));
        f32x16 a;
#pragma unroll
        for (int e = 0; e < 16; ++e) a[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], a, 0, 0, 0);
        s[kt] = a;
    }
    // key j of the last tile counts for this lane's query when j <= r (the diagonal tile) or when it is a token
    auto counts = [&](int e) {
        const int j = (e & 3) + 8 * (e >> 2) + 4 * hh;
        return CAUSAL ? j <= r : 32 * (NT - 1) + j < T;
    };
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT - 1; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[kt][e]);
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, counts(e) ? s[NT - 1][e] : -INFINITY);
    mx = fmaxf(mx, other_half(mx));  // the first key of the last tile (lower half, e = 0) counts for every query: mx is a score
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
            if (kt == NT - 1) pv = counts(e) ? pv : 0.f;
            sum += pv;
            pf[j] = (bf16_t)pv;
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const s16x8 vf = read_vt_frag(Vl + I * 16 * ATTN_ROWB + (db ? v_off1 : v_off0), ATTN_ROWB);
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), pf, o[db], 0, 0, 0);
        }
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

// qkv [n * T, 3 * 64 H] (Q | K | V, Q pre-scaled) -> out [n * T, 64 H]; items = n * H
template <int T, bool CAUSAL>
__global__ __launch_bounds__(64 * ((T + 31) / 32)) void attn_short(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int items,
                                                                   const int H, const int only_block) {
    constexpr int WAVES = (T + 31) / 32;
    static_assert(!CAUSAL || WAVES == 3, "attn_short: the causal form dispatches three query blocks");
    constexpr int KV_BYTES = WAVES * 32 * ATTN_ROWB;  // WAVES key tiles of 32 rows
    constexpr int NPIECE = WAVES * 4;                  // LDS-DMA pieces of 8 rows for K, as many for V
    __shared__ __attribute__((aligned(16))) char lds[2 * KV_BYTES];  // K | V of the current item
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = H * VIT_DH;
    const size_t qkv_ld = (size_t)3 * D * 2;  // bytes per row of the fused activation
    const int q = wave * 32 + (lane & 31), hh = lane >> 5;
    const int qc = min(q, T - 1);
    const bool mine = CAUSAL || only_block < 0 || only_block == wave;  // wave-uniform
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int seq = it / H, h = it - seq * H;
        const char* hb = (const char*)qkv + (size_t)seq * T * qkv_ld + h * ATTN_ROWB;
        if (it != (int)blockIdx.x) S_BARRIER();  // every wave is done with the previous item's K / V
        for (int p = wave; p < 2 * NPIECE; p += WAVES) {  // both swizzles are applied to the source address
            const bool isv = p >= NPIECE;
            const int pp = isv ? p - NPIECE : p;
            lds_dma16(kv_piece_src<T - 1>(hb, qkv_ld, D, isv, pp, lane), lds + (isv ? KV_BYTES : 0) + pp * 1024);
        }
        bf16x8 qf[4];
        {
            const char* qp = hb + (size_t)qc * qkv_ld + hh * 16;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 32);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces have landed
        S_BARRIER();                                                  // everybody's
        bf16_t* op = out + ((size_t)seq * T + qc) * D + h * VIT_DH;
        const bool store = q < T;
        if (mine) {
            if constexpr (!CAUSAL) short_block<T, CAUSAL, 0>(lds, lds + KV_BYTES, qf, lane, op, store);  // every block multiplies every tile
            else if (wave == 0) short_block<T, CAUSAL, 0>(lds, lds + KV_BYTES, qf, lane, op, store);
            else if (wave == 1) short_block<T, CAUSAL, 1>(lds, lds + KV_BYTES, qf, lane, op, store);
            else short_block<T, CAUSAL, 2>(lds, lds + KV_BYTES, qf, lane, op, store);
        }
    }
}

static_assert(count_attn(ATTN_SHORT) == 3 && attn_row(ATTN_SHORT, TXT_T, true) && attn_row(ATTN_SHORT, 50) && attn_row(ATTN_SHORT, TXT_T64),
              "attn_short: instantiate the kernel for every layout of this family");

}  // namespace

hipError_t launch_attention_exact(const void* qkv, void* out, int n, int tokens, bool causal, int heads, hipStream_t s, int only_block) {
    const TokenLayout* L = find_layout(tokens, causal);
    if (!L || L->attn == ATTN_LONG || !L->has_heads(heads) || !L->takes_block(only_block)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    if (L->attn == ATTN_MID) return launch_attn_mid(qkv, out, n, heads, s, only_block);
    const int64_t items = (int64_t)n * heads;
    if (items > 0x7fffffff) return hipErrorInvalidValue;
    const int grid = items < 1024 ? (int)items : 1024;  // persistent: up to four workgroups per CU walk the items
    const dim3 waves(64 * L->blocks);  // a wave per query block
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), waves, 0, s, (const bf16_t*)qkv, (bf16_t*)out, (int)items, heads, only_block); };
    if (tokens == TXT_T) go(attn_short<TXT_T, true>);
    else if (tokens == 50) go(attn_short<50, false>);
    else go(attn_short<TXT_T64, false>);
    return hipGetLastError();
}
