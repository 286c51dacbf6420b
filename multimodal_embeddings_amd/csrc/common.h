// Shared device helpers for the gfx950 (CDNA4) kernels.  64-wide wavefronts throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// Experiment switches -- environment variables that select ablations of the stamped kernel builds (MME_ATTN_DEBUG,
// MME_TATTN_DEBUG) and produce wrong results on purpose -- exist only in the diagnostic build (`python -m
// multimodal_embeddings_amd.build --diag` -> libmme_diag.so, -DMME_DIAG): a stray variable in a user's environment cannot
// change what libmme.so computes.
#include <stdlib.h>
#ifdef MME_DIAG
static inline const char* diag_env(const char* name) { return getenv(name); }
#else
static inline const char* diag_env(const char*) { return nullptr; }
#endif

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// ViT/16 @224 geometry.  What every supported encoder shares is fixed at compile time, so that the index computations
// of the attention kernel, the patch emitter and the patch-embed epilogue fold to constants: 197 tokens of 16 x 16
// patches, heads of 64.  Width, depth, head count and MLP size belong to the weights a context was loaded with
// (ctx.h, VitGeom); the row kernels and the attention kernel are instantiated per supported width (384, 768, 1024 =
// 6, 12, 16 heads).  VIT_D / VIT_H / VIT_F / VIT_L are ViT-B/16, the geometry of a context before any load.
constexpr int VIT_D = 768;
constexpr int VIT_T = 197;
constexpr int VIT_NP = 196;
constexpr int VIT_H = 12;
constexpr int VIT_DH = 64;
constexpr int VIT_F = 3072;
constexpr int VIT_L = 12;
constexpr int VIT_GRID = 14;
constexpr int VIT_PATCH = 16;
constexpr int VIT_IMG = 224;
constexpr int VIT_PATCH_DIM = 3 * VIT_PATCH * VIT_PATCH;  // im2col row of one patch: K of the patch-embed GEMM (768 at every width)
constexpr int VIT_MAX_L = 64;                             // the guard-word table of a pass (ctx.h, attn_guard)
constexpr int VIT_MAX_F = 8192;
// the widths the row kernels and the attention kernel are instantiated for
constexpr bool vit_width_built(int d) { return d == 384 || d == 768 || d == 1024; }

// CLIP text tower: 77 tokens (CLIPTextConfig.max_position_embeddings), heads of 64 as above; its row kernels and its
// causal attention kernel run the widths 512, 768 and 1024 (8, 12, 16 heads).  512 is no width of the image path.
constexpr int TXT_T = 77;
constexpr int TXT_MAX_VOCAB = 65536;
constexpr int TXT_T64 = 64;                  // SigLIP text towers: 64 positions
constexpr int TXT_MAX_VOCAB_SIGLIP = 262144;  // SigLIP 32000, SigLIP 2 256000
constexpr bool text_width_built(int d) { return d == 512 || d == 768 || d == 1024; }
#include "layouts.h"  // the table of token layouts: one row for each of the sequence lengths above and below

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// 16-byte asynchronous global -> LDS copy (LDS-DMA).  The LDS destination is the
// wave-uniform base + lane*16; only the SOURCE address is per lane.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gsrc, (LDS_AS void*)lds_wave_base, 16, 0, 0);
}

// XCD-aware bijective block remap: consecutive logical tiles land on one XCD (its own
// L2), whatever the grid size.  `orig % 8` labels blocks sharing an XCD.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (orig >> 3);
}
