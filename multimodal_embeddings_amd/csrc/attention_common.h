// Device pieces the attention kernels share: attention.hip (197 tokens), attention_short.hip (77 and 50 tokens) and, where
// its LDS images allow, attention_tiles.hip.  Everything here is forced inline.  A kernel adopts a piece only where its
// instruction stream stays what it was with the piece written out (tools/kernel_streams.py; DESIGN.md, "attention
// kernels, one set of pieces"), so a few keep their own text: attention_short.hip its K-fragment read, attn_fwd_tiles its
// output store, and the two guarded fast forms their "is the total of O finite" reduction (no shape of it came through).
//
// LDS images of the dh = 64 kernels: K rows of 128 B with chunk ^= (row >> 1) & 7 (conflict-free ds_read_b128), V rows of
// 128 B with the two 64-byte halves swapped when bit 1 of the row is set (conflict-free transposed reads); both swizzles
// are applied to the LDS-DMA source address.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int ATTN_ROWB = VIT_DH * 2;  // 128-byte K / V rows in LDS (dh = 64)

#define S_BARRIER() asm volatile("s_barrier" ::: "memory")

// the other half of the wave (lane ^ 32) holds the other keys of this lane's query: exchange by ONE v_permlane32_swap (vector
// ALU) instead of __shfl_xor's ds_bpermute round trip through the LDS, whose latency sits on the head's critical path
__device__ __forceinline__ float other_half(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    // after the swap sw[0] = {lo, lo}, sw[1] = {hi, hi}: the value this lane did not have is the one that differs
    const float a = __uint_as_float(sw[0]), b = __uint_as_float(sw[1]);
    return (threadIdx.x & 32) ? a : b;
}

// LDS-DMA of K and V of one (sequence, head) item, in pieces of 8 rows x 128 B: the K pieces 0 .. npiece - 1, then V's.
// Source of this lane's 16 bytes of piece pp of K or V (isv), both swizzles applied: hb = the item's Q row 0, ld = bytes per
// row of the fused activation [., 3 D] (Q | K | V); rows past `last` receive clamped copies of row `last` (finite).
template <int last>
__device__ __forceinline__ const char* kv_piece_src(const char* hb, const size_t ld, const int D, const bool isv, const int pp, const int lane) {
    const int row = pp * 8 + (lane >> 3);
    const int slot = lane & 7;
    const int chunk = isv ? (slot ^ (((row >> 1) & 1) << 2)) : (slot ^ ((row >> 1) & 7));
    return hb + (size_t)min(row, last) * ld + (isv ? 2 : 1) * D * 2 + chunk * 16;
}
// One piece: 64 lanes x 16 bytes from src to the wave-uniform LDS address ldst + 16 lane.  Through inline asm, so that hipcc
// does not know these loads write LDS: told through the builtin (glds16) it orders every later LDS read behind them with
// `s_waitcnt vmcnt(0)` -- in the middle of an item, where that also waits for the Q prefetch and the previous item's
// stores.  The ordering that is needed (pieces landed before they are read) is the caller's counted wait + barrier.
__device__ __forceinline__ void lds_dma16(const char* src, char* ldst) {
    const unsigned dst = (unsigned)(size_t)(LDS_AS char*)ldst;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst))
                 : "memory");
}
// A operands of S^T = K . Q^T for key tile kt: this lane's key row 32 kt + r, k-step ks = its chunk 2 ks + hh (un-swizzled)
// (r = lane & 31, hh = lane >> 5), through the swizzle ksw = (r >> 1) & 7
__device__ __forceinline__ void read_k_frag(const char* Kl, const int kt, const int r, const int hh, const int ksw, bf16x8 (&dst)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) dst[ks] = *(const bf16x8*)(Kl + (kt * 32 + r) * ATTN_ROWB + (((2 * ks + hh) ^ ksw) << 4));
}

// Transposed V reads (ds_read_b64_tr_b16) from the row-major image.  Lane roles: group g of 16 lanes, lane 4 q + p supplies
// row q, cols 4 p .. 4 p + 3; the offset addresses head dims 32 db .. 32 db + 31 through the half swap of this lane's row.
__device__ __forceinline__ int vt_lane_off(const int lane, const int db) {
    const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    const int vflag = (tq >> 1) & 1;  // bit 1 of the row this lane addresses: selects the swapped half
    const int row_off = (4 * (g >> 1) + tq) * ATTN_ROWB + (16 * (g & 1) + 4 * tp) * 2;
    return row_off + ((db ^ vflag) << 6);
}
// V^T fragment at va: 16 keys (two transposed reads 8 rows of `pitch` bytes apart) x the lane's 4 head dims
__device__ __forceinline__ s16x8 read_vt_frag(const char* va, const int pitch) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)va);
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(va + 8 * pitch));
    return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Row groups rp and rp + 1 of one 32-dim block of O^T, scaled and rounded: o[4 rg + j] = O[q][32 db + 8 rg + 4 hh + j].
// The lower lane half keeps group rp and receives the upper half's group rp (dims +4 .. +7), the upper half keeps group
// rp + 1 and receives the lower half's (dims +0 .. +3): 16 bytes per lane, to be stored at dim 32 db + 8 (rp + hh).
__device__ __forceinline__ uint4 paired_o(const f32x16 o, const int rp, const float inv) {
    bf16x4 t0, t1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t0[j] = (bf16_t)(o[rp * 4 + j] * inv);
        t1[j] = (bf16_t)(o[(rp + 1) * 4 + j] * inv);
    }
    const uint2 u0 = __builtin_bit_cast(uint2, t0), u1 = __builtin_bit_cast(uint2, t1);
    const auto ax = __builtin_amdgcn_permlane32_swap(u0.x, u1.x, false, false);
    const auto ay = __builtin_amdgcn_permlane32_swap(u0.y, u1.y, false, false);
    return make_uint4(ax[0], ay[0], ax[1], ay[1]);
}
